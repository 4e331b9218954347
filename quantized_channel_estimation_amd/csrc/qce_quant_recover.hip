// The per-component recovery algebra of the quantised M-step (reference gmm_cplx_quant.py:773-853, :880-945;
// cov_est_quant.py:31-88 est_cov_from_quant; utils.py:651-700 gauss_newt_solve) on the device, FP64:
//
// k_qr_fit: the scalar Gauss-Newton variance fits, one thread per (component k, dimension d).  With the 2T residuals
//   f = erf(t / (sqrt 2 s)) - p and J = -sqrt(2 / pi) t exp(-t^2 / (2 s)) / s^2 (the exponent as the reference has
//   it) a step is dx = -(J . f) / (J . J) -- lstsq for one column, 0 when J . J is exactly 0 -- until |dx| <= 1e-5 or
//   100 steps; s2 = max(2 s^2, 0).  The reference restarts a fit whose |s| leaves [0.1, 10] from numpy's global
//   generator: such a thread, or one that meets a non-finite value, stops with status 1 and the host redoes the entry.
//
// k_qr_clip: C <- V max(L, floor) V^H of a Hermitian D x D matrix (D <= 64; its lower triangle is read, as eigh does),
//   one workgroup per component, by parallel cyclic two-sided Jacobi with A and V in LDS.  The pairs of a step come
//   from a round-robin tournament over n = D + (D odd) indices (an odd D gets a bye index); a step is three phases
//   separated by barriers: every pair takes its rotation J = [[c, s w], [-s conj(w), c]] from the current 2 x 2
//   block, every pair rotates its two columns of A and V (X <- X J), every pair rotates its two rows of A
//   (A <- J^H A; the block itself is written as diag(a - t g, b + t g)).  A sweep is n - 1 steps; the iteration stops
//   when the off-diagonal Frobenius norm, summed from the off-diagonal entries themselves (the difference
//   ||A||^2 - ||diag||^2 cancels at 1e-16 ||A||^2 and would stop near 1e-8), is <= 1e-14 ||C||_F, or after 30 sweeps
//   with status 1 (the host then clips that component with eigh).  Rows have an odd stride, so a column walk is free
//   of bank conflicts.  Fixed order, no atomics: bit-reproducible.  The load stage fuses the element-wise preparation
//   of the branches (arcsine law, r corr r scaling, a diagonal shift), the store stage a diagonal shift.
#include "qce_capi.h"
#include "qce_common.h"

#pragma clang fp contract(off)

namespace {

constexpr double FIT_TOL = 1e-5;
constexpr int FIT_MAXITS = 100;
constexpr double OFF_TOL2 = 1e-28;  // (1e-14)^2: the norms are compared squared
constexpr int CLIP_MAX_SWEEPS = 30;
constexpr int CLIP_MAX_D = 64;
constexpr int CLIP_THREADS = 512;

__global__ __launch_bounds__(256) void k_qr_fit(int K, int D, int T, const double* __restrict__ probs,
                                                const double* __restrict__ nk, const double* __restrict__ thr,
                                                const double* __restrict__ x0, double* __restrict__ s2,
                                                int* __restrict__ status, int* __restrict__ iters) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)K * D) return;
  const double n = nk[e / D];
  const double lo = 1.0 / n, hi = (n - 1.0) / n;
  const double* p = probs + e * T * 2;
  const double c = sqrt(2.0 / M_PI), r2 = sqrt(2.0);
  double dx = 1.0, s = x0[e];
  int i = 0, bad = 0;
  while (i < FIT_MAXITS && fabs(dx) > FIT_TOL) {
    if (fabs(s) < 0.1 || fabs(s) > 10.0) {  // the reference's restart branches
      bad = 1;
      break;
    }
    const double den = r2 * s, two_s = 2.0 * s, ss = s * s;
    double jj = 0.0, jf = 0.0;
    for (int part = 0; part < 2; ++part) {  // real-part probabilities first, then the imaginary-part ones
      for (int t = 0; t < T; ++t) {
        const double th = thr[t];
        double pv = p[2 * t + part];  // NaN stays NaN (np.clip) and ends the fit below
        pv = pv < lo ? lo : pv;
        pv = pv > hi ? hi : pv;
        const double f = erf(th / den) - pv;
        const double J = -c * th * exp(-(th * th) / two_s) / ss;
        jj += J * J;
        jf += J * f;
      }
    }
    dx = jj == 0.0 ? 0.0 : -jf / jj;
    s += dx;
    ++i;
    if (!(isfinite(dx) && isfinite(s))) {
      bad = 1;
      break;
    }
  }
  double v = s * s;
  if (v != v) v = 1.0;
  v = 2.0 * v;
  s2[e] = bad ? 1.0 : (v > 0.0 ? v : 0.0);
  status[e] = bad;
  iters[e] = i;
}

struct ClipRot {
  int p, q;      // p < 0: no rotation (a bye, or an off-diagonal entry that is exactly 0)
  double cs;
  double2 sw;    // s w, w = A[p][q] / |A[p][q]|
  double app, aqq;
};

// sum of v over the workgroup in a fixed order (a tree over the threads); every thread returns the total
QCE_DEV double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous use of red is over
  red[tid] = v;
  __syncthreads();
  for (int h = CLIP_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// sum |A[i][j]|^2 over i != j (all == false) or all entries; each thread its strided share in ascending order
QCE_DEV double norm2(const double2* A, int D, int LD, bool all, double* red) {
  double acc = 0.0;
  for (int e = threadIdx.x; e < D * D; e += CLIP_THREADS) {
    const int i = e / D, j = e - i * D;
    const double2 a = A[i * LD + j];
    if (all || i != j) acc += a.x * a.x + a.y * a.y;
  }
  return block_sum(acc, red);
}

__global__ __launch_bounds__(CLIP_THREADS) void k_qr_clip(int D, double floor, int prep, double diag_pre,
                                                          double diag_post, const double2* __restrict__ in,
                                                          const double* __restrict__ s2, double2* __restrict__ out,
                                                          int* __restrict__ status, int* __restrict__ sweeps_out) {
  extern __shared__ __attribute__((aligned(16))) char qr_smem[];
  const int LD = D | 1;          // odd row stride (in 16 B elements)
  const int n = D + (D & 1);     // tournament size
  const int m = n >> 1;          // pairs per step
  double2* A = reinterpret_cast<double2*>(qr_smem);
  double2* V = A + D * LD;
  double* red = reinterpret_cast<double*>(V + D * LD);
  double* lam = red + CLIP_THREADS;
  ClipRot* rot = reinterpret_cast<ClipRot*>(lam + CLIP_MAX_D);
  const int tid = threadIdx.x, k = blockIdx.x;
  const double2* Ck = in + (long long)k * D * D;
  const double* sk = s2 ? s2 + (long long)k * D : nullptr;

  // load: the lower triangle, mirrored; the branch's element-wise preparation
  for (int e = tid; e < D * D; e += CLIP_THREADS) {
    const int i = e / D, j = e - i * D;
    double2 a = i >= j ? Ck[i * D + j] : cconj(Ck[j * D + i]);
    if (prep >= QCE_CLIP_SIN) a = make_double2(sin(M_PI / 2 * a.x), sin(M_PI / 2 * a.y));
    if (prep == QCE_CLIP_SIN_SCALED) {
      const double ri = sqrt(sk[i]), rj = sqrt(sk[j]);
      a = make_double2(ri * a.x * rj, ri * a.y * rj);
    }
    if (i == j) a = make_double2(a.x + diag_pre, 0.0);
    A[i * LD + j] = a;
    V[i * LD + j] = make_double2(i == j ? 1.0 : 0.0, 0.0);
  }
  __syncthreads();
  const double total2 = norm2(A, D, LD, true, red);

  int sweeps = 0, bad = 0;
  while (!(norm2(A, D, LD, false, red) <= OFF_TOL2 * total2)) {  // uniform: every thread holds the same sums
    if (sweeps == CLIP_MAX_SWEEPS) {
      bad = 1;
      break;
    }
    for (int r = 0; r < n - 1; ++r) {
      // phase 1: the rotations of this step's pairs from the current 2 x 2 blocks
      if (tid < m) {
        int a = tid == 0 ? n - 1 : (r + tid) % (n - 1);
        int b = tid == 0 ? r : (r - tid + n - 1) % (n - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        ClipRot R;
        R.p = -1;
        R.q = q;
        R.cs = 1.0;
        R.sw = make_double2(0.0, 0.0);
        R.app = R.aqq = 0.0;
        if (q < D) {
          const double app = A[p * LD + p].x, aqq = A[q * LD + q].x;
          const double2 c = A[p * LD + q];
          const double g = hypot(c.x, c.y);
          if (g != 0.0) {
            const double tau = (aqq - app) / (2.0 * g);
            const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
            const double cs = 1.0 / sqrt(1.0 + t * t);
            const double sn = t * cs;
            R.p = p;
            R.cs = cs;
            R.sw = make_double2(sn * (c.x / g), sn * (c.y / g));
            R.app = app - t * g;
            R.aqq = aqq + t * g;
          }
        }
        rot[tid] = R;
      }
      __syncthreads();
      // phase 2: columns p, q of A and V (X <- X J); lanes walk the rows
      for (int e = tid; e < m * D; e += CLIP_THREADS) {
        const int pr = e / D, i = e - pr * D;
        const ClipRot R = rot[pr];
        if (R.p < 0) continue;
        const double2 swc = cconj(R.sw);
        double2* x = A + i * LD;
        double2 xp = x[R.p], xq = x[R.q];
        x[R.p] = csub(cscale(xp, R.cs), cmul(xq, swc));
        x[R.q] = cadd(cmul(xp, R.sw), cscale(xq, R.cs));
        x = V + i * LD;
        xp = x[R.p];
        xq = x[R.q];
        x[R.p] = csub(cscale(xp, R.cs), cmul(xq, swc));
        x[R.q] = cadd(cmul(xp, R.sw), cscale(xq, R.cs));
      }
      __syncthreads();
      // phase 3: rows p, q of A (A <- J^H A); lanes walk the columns
      for (int e = tid; e < m * D; e += CLIP_THREADS) {
        const int pr = e / D, j = e - pr * D;
        const ClipRot R = rot[pr];
        if (R.p < 0) continue;
        double2* xp = A + R.p * LD + j;
        double2* xq = A + R.q * LD + j;
        const double2 vp = *xp, vq = *xq;
        double2 np_ = csub(cscale(vp, R.cs), cmul(R.sw, vq));
        double2 nq_ = cadd(cmul(cconj(R.sw), vp), cscale(vq, R.cs));
        if (j == R.p) {
          np_ = make_double2(R.app, 0.0);
          nq_ = make_double2(0.0, 0.0);
        } else if (j == R.q) {
          np_ = make_double2(0.0, 0.0);
          nq_ = make_double2(R.aqq, 0.0);
        }
        *xp = np_;
        *xq = nq_;
      }
      __syncthreads();
    }
    ++sweeps;
  }

  // store: W = V max(L, floor) into A, then C = W V^H (upper triangle, mirrored)
  if (tid < D) {
    const double l = A[tid * LD + tid].x;
    lam[tid] = l < floor ? floor : l;
  }
  __syncthreads();
  for (int e = tid; e < D * D; e += CLIP_THREADS) {
    const int i = e / D, l = e - i * D;
    A[i * LD + l] = cscale(V[i * LD + l], lam[l]);
  }
  __syncthreads();
  double2* Ok = out + (long long)k * D * D;
  for (int e = tid; e < D * D; e += CLIP_THREADS) {
    const int i = e / D, j = e - i * D;  // lanes walk j: rows j of V, bank-conflict free by the odd stride
    if (j < i) continue;
    double2 acc = make_double2(0.0, 0.0);
    const double2* w = A + i * LD;
    const double2* v = V + j * LD;
    for (int l = 0; l < D; ++l) acc = cadd(acc, cmulc(w[l], v[l]));
    if (i == j) {
      Ok[i * D + i] = make_double2(acc.x + diag_post, 0.0);
    } else {
      Ok[i * D + j] = acc;
      Ok[j * D + i] = cconj(acc);
    }
  }
  if (tid == 0) {
    status[k] = bad;
    sweeps_out[k] = sweeps;
  }
}

size_t clip_lds_bytes(int D) {
  const size_t LD = (size_t)(D | 1);
  return 2 * sizeof(double2) * D * LD + sizeof(double) * (CLIP_THREADS + CLIP_MAX_D) +
         sizeof(ClipRot) * (CLIP_MAX_D / 2);
}

}  // namespace

extern "C" int qce_quant_variance_fit(const double* probs, const double* nk, const double* thresholds, int T,
                                      const double* x0, int K, int D, double* s2_out, int32_t* status_out,
                                      int32_t* iters_out, int device, int io, void* stream) {
  if (K < 1 || D < 1 || T < 1 || !probs || !nk || !thresholds || !x0 || !s2_out || !status_out || !iters_out)
    return qce_set_error(QCE_EARG, "quant_variance_fit: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "quant_variance_fit: bad io");
  if ((long long)K * D > (1LL << 30)) return qce_set_error(QCE_ENOTIMPL, "quant_variance_fit: K D <= 2^30");
  for (int t = 0; t < T; ++t)
    if (!(thresholds[t] > 0.0) || (t > 0 && !(thresholds[t] > thresholds[t - 1])))
      return qce_set_error(QCE_EARG, "quant_variance_fit: thresholds must be positive and ascending");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t nE = (size_t)K * D, nP = nE * T * 2;
  DevBuf<double> dthr, dprobs, dnk, dx0, ds2;
  DevBuf<int> dstatus, diters;
  HIPCHK(dthr.ensure(T));
  HIPCHK(hipMemcpyAsync(dthr.p, thresholds, sizeof(double) * T, hipMemcpyHostToDevice, st));
  const double *p = probs, *n = nk, *x = x0;
  double* s2 = s2_out;
  int *status = status_out, *iters = iters_out;
  if (io == QCE_IO_HOST) {
    HIPCHK(dprobs.ensure(nP));
    HIPCHK(dnk.ensure(K));
    HIPCHK(dx0.ensure(nE));
    HIPCHK(ds2.ensure(nE));
    HIPCHK(dstatus.ensure(nE));
    HIPCHK(diters.ensure(nE));
    HIPCHK(hipMemcpyAsync(dprobs.p, probs, sizeof(double) * nP, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dnk.p, nk, sizeof(double) * K, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dx0.p, x0, sizeof(double) * nE, hipMemcpyHostToDevice, st));
    p = dprobs.p;
    n = dnk.p;
    x = dx0.p;
    s2 = ds2.p;
    status = dstatus.p;
    iters = diters.p;
  }
  hipLaunchKernelGGL(k_qr_fit, dim3((unsigned)((nE + 255) / 256)), dim3(256), 0, st, K, D, T, p, n, dthr.p, x, s2,
                     status, iters);
  HIPCHK(hipGetLastError());
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(s2_out, s2, sizeof(double) * nE, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status_out, status, sizeof(int) * nE, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(iters_out, iters, sizeof(int) * nE, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // the staging above is freed on return
  return QCE_OK;
}

extern "C" int qce_herm_eig_clip(const double* C, int K, int D, double floor, int prep, const double* s2,
                                 double diag_pre, double diag_post, double* out, int32_t* status_out,
                                 int32_t* sweeps_out, int device, int io, void* stream) {
  if (K < 1 || D < 1 || !C || !out || !status_out || !sweeps_out)
    return qce_set_error(QCE_EARG, "herm_eig_clip: bad arguments");
  if (prep != QCE_CLIP_PLAIN && prep != QCE_CLIP_SIN && prep != QCE_CLIP_SIN_SCALED)
    return qce_set_error(QCE_EARG, "herm_eig_clip: bad prep");
  if (prep == QCE_CLIP_SIN_SCALED && !s2) return qce_set_error(QCE_EARG, "herm_eig_clip: the scaled prep needs s2");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "herm_eig_clip: bad io");
  if (D > CLIP_MAX_D) return qce_set_error(QCE_ENOTIMPL, "herm_eig_clip: D <= 64");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t nC = (size_t)K * D * D, nS = (size_t)K * D;
  DevBuf<double2> dC, dout;
  DevBuf<double> ds2;
  DevBuf<int> dstatus, dsweeps;
  const double2* c = (const double2*)C;
  const double* s = prep == QCE_CLIP_SIN_SCALED ? s2 : nullptr;
  double2* o = (double2*)out;
  int *status = status_out, *sweeps = sweeps_out;
  if (io == QCE_IO_HOST) {
    HIPCHK(dC.ensure(nC));
    HIPCHK(dout.ensure(nC));
    HIPCHK(dstatus.ensure(K));
    HIPCHK(dsweeps.ensure(K));
    HIPCHK(hipMemcpyAsync(dC.p, C, sizeof(double2) * nC, hipMemcpyHostToDevice, st));
    if (s) {
      HIPCHK(ds2.ensure(nS));
      HIPCHK(hipMemcpyAsync(ds2.p, s, sizeof(double) * nS, hipMemcpyHostToDevice, st));
      s = ds2.p;
    }
    c = dC.p;
    o = dout.p;
    status = dstatus.p;
    sweeps = dsweeps.p;
  }
  const size_t lds = clip_lds_bytes(D);
  if (lds > (32u << 10))
    HIPCHK(hipFuncSetAttribute((const void*)k_qr_clip, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_qr_clip, dim3(K), dim3(CLIP_THREADS), lds, st, D, floor, prep, diag_pre, diag_post, c, s, o,
                     status, sweeps);
  HIPCHK(hipGetLastError());
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(out, o, sizeof(double2) * nC, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status_out, status, sizeof(int) * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(sweeps_out, sweeps, sizeof(int) * K, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // the staging above is freed on return
  return QCE_OK;
}
