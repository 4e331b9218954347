// C ABI of libqce.so, the entry points that run beside the estimator proper: observation / error metrics
// (qce_observe, qce_sq_error), EM steps, per-sample filters / LS, the SCM channel generator, rate bounds and the VAE
// estimator.  Most take no model; those that do read its tables through the helpers of qce_capi.h.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qce_capi.h"
#include "qce_common.h"

// The constants of k_vae for one (snr, n_bits, pilot vector); the caller has checked N and P.
int vae_lmmse_args(const char* who, int N, int P, const double* x_cplx, double snr_db, double n_bits, QceVaeArgs* a) {
  a->N = N;
  a->P = P;
  a->n_bits = 0;
  a->delta = 0.0;
  if (n_bits == 1.0) a->kind = 0;
  else if (isinf(n_bits) && n_bits > 0) a->kind = 2;
  else {
    a->kind = 1;
    a->n_bits = (int)n_bits;
    if (!(n_bits >= 2.0) || (double)a->n_bits != n_bits) return qce_set_error(QCE_EARG, std::string(who) + ": n_bits must be an integer >= 1 or inf");
    if (a->n_bits > QCE_MAX_UNIFORM_BITS)
      return qce_set_error(QCE_ENOTIMPL, std::string(who) + ": uniform quantisers up to " + std::to_string(QCE_MAX_UNIFORM_BITS) + " bits");
    a->delta = uniform_step(snr_db, a->n_bits);
  }
  // the reference builds these constants from torch.tensor(np.pi), a float32 tensor (vae.py:403, :410,
  // uniform_quantizer.py:79, :86)
  const float pi_f = (float)M_PI;
  a->k1 = (double)sqrtf(2.0f / pi_f);
  a->k2 = (double)((float)a->delta / sqrtf(pi_f));
  a->k3 = (double)(2.0f / pi_f);
  a->s2 = pow(10.0, -snr_db / 10.0);
  for (int p = 0; p < QCE_VAE_MAX_PILOTS; ++p)
    a->x[p] = p < P ? make_double2(x_cplx[2 * p], x_cplx[2 * p + 1]) : make_double2(0.0, 0.0);
  a->lv_f32 = 0;
  a->TS = 0;
  return QCE_OK;
}

extern "C" {

int qce_observe(const double* h, int64_t B, int N, const double* A, int M, double noise_scale, int noise_kind,
                const double* noise, uint64_t seed, uint64_t offset, double n_bits, const double* thresholds,
                const double* labels, int n_levels, double* y_out, int device, int io, void* stream) {
  if (B < 0 || N < 1 || (A && M < 1) || (!A && M != N)) return qce_set_error(QCE_EARG, "observe: bad shape");
  if (noise_kind < 0 || noise_kind > 2 || (noise_kind == 1 && !noise)) return qce_set_error(QCE_EARG, "observe: bad noise");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "observe: bad io");
  if (B > 0 && (!h || !y_out)) return qce_set_error(QCE_EARG, "observe: null buffer");
  int kind;
  if (n_bits == 1.0) kind = 0;
  else if (isinf(n_bits) && n_bits > 0) kind = 2;
  else {
    kind = 1;
    if (!thresholds || !labels || n_levels < 2 || n_levels > 256)
      return qce_set_error(QCE_EARG, "observe: multi-bit quantisation needs thresholds (L-1) and labels (L), 2 <= L <= 256");
    for (int i = 1; i < n_levels - 1; ++i)
      if (!(thresholds[i] >= thresholds[i - 1])) return qce_set_error(QCE_EARG, "observe: thresholds must be increasing");
  }
  if (B == 0) return QCE_OK;
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t ny = (size_t)B * M, nh = (size_t)B * N;
  QceObserveArgs a;
  a.B = B;
  a.M = M;
  a.N = N;
  a.noise = noise_kind;
  a.noise_scale = noise_scale;
  a.seed = seed;
  a.offset = offset;
  a.kind = kind;
  a.nthr = kind == 1 ? n_levels - 1 : 0;
  {
    StreamScratch sc(st);
    void* p;
    a.A = nullptr;
    if (A) {
      HIPCHK(sc.get(&p, sizeof(double2) * (size_t)M * N));
      HIPCHK(hipMemcpyAsync(p, A, sizeof(double2) * (size_t)M * N, hipMemcpyHostToDevice, st));
      a.A = (const double2*)p;
    }
    a.thr = a.lab = nullptr;
    if (kind == 1) {
      HIPCHK(sc.get(&p, sizeof(double) * (size_t)(2 * n_levels - 1)));
      HIPCHK(hipMemcpyAsync(p, thresholds, sizeof(double) * (n_levels - 1), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync((double*)p + n_levels - 1, labels, sizeof(double) * n_levels, hipMemcpyHostToDevice, st));
      a.thr = (const double*)p;
      a.lab = (const double*)p + n_levels - 1;
    }
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&p, sizeof(double2) * nh));
      HIPCHK(hipMemcpyAsync(p, h, sizeof(double2) * nh, hipMemcpyHostToDevice, st));
      a.h = (const double2*)p;
      a.w = nullptr;
      if (noise_kind == 1) {
        HIPCHK(sc.get(&p, sizeof(double2) * ny));
        HIPCHK(hipMemcpyAsync(p, noise, sizeof(double2) * ny, hipMemcpyHostToDevice, st));
        a.w = (const double2*)p;
      }
      HIPCHK(sc.get(&p, sizeof(double2) * ny));
      a.y = (double2*)p;
    } else {
      a.h = (const double2*)h;
      a.w = (const double2*)noise;
      a.y = (double2*)y_out;
    }
    HIPCHK(qce_launch_observe(a, st));
    if (io == QCE_IO_HOST) HIPCHK(hipMemcpyAsync(y_out, a.y, sizeof(double2) * ny, hipMemcpyDeviceToHost, st));
  }
  if (io == QCE_IO_HOST) HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_observe_randsnr(const double* h, int64_t B, int N, const double* A, int M, int S, const double* noise_scales,
                        const double* cdf, const int32_t* snr_index_in, int32_t* snr_index_out, int noise_kind,
                        const double* noise, uint64_t seed, uint64_t row_offset, double n_bits,
                        const double* thresholds, const double* labels, int n_levels, int out_kind, void* out,
                        int device, int io, void* stream) {
  if (B < 0 || N < 1 || (A && M < 1) || (!A && M != N)) return qce_set_error(QCE_EARG, "observe_randsnr: bad shape");
  if (S < 1 || S > QCE_ROWS_MAX_SNRS || !noise_scales)
    return qce_set_error(QCE_EARG, "observe_randsnr: 1 to " + std::to_string(QCE_ROWS_MAX_SNRS) + " SNRs with their noise scales");
  if (noise_kind < 0 || noise_kind > 2 || (noise_kind == 1 && !noise)) return qce_set_error(QCE_EARG, "observe_randsnr: bad noise");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "observe_randsnr: bad io");
  if (out_kind < QCE_OUT_Y || out_kind > QCE_OUT_FEATURES_DFT) return qce_set_error(QCE_EARG, "observe_randsnr: bad output kind");
  if (B > 0 && (!h || !out || !snr_index_out)) return qce_set_error(QCE_EARG, "observe_randsnr: null buffer");
  if (cdf)
    for (int i = 0; i < S; ++i)
      if (!(cdf[i] >= (i ? cdf[i - 1] : 0.0))) return qce_set_error(QCE_EARG, "observe_randsnr: cdf must be non-decreasing from 0");
  int kind;
  if (n_bits == 1.0) kind = 0;
  else if (isinf(n_bits) && n_bits > 0) kind = 2;
  else {
    kind = 1;
    if (!thresholds || !labels || n_levels < 2 || n_levels > 256)
      return qce_set_error(QCE_EARG, "observe_randsnr: multi-bit quantisation needs thresholds (S, L-1) and labels (S, L), 2 <= L <= 256");
    for (int s = 0; s < S; ++s)
      for (int i = 1; i < n_levels - 1; ++i)
        if (!(thresholds[(size_t)s * (n_levels - 1) + i] >= thresholds[(size_t)s * (n_levels - 1) + i - 1]))
          return qce_set_error(QCE_EARG, "observe_randsnr: thresholds of SNR " + std::to_string(s) + " must be increasing");
  }
  if (out_kind != QCE_OUT_Y) {
    if (!qce_observe_rows_feature_shape(N))
      return qce_set_error(QCE_ENOTIMPL, "observe_randsnr: features need n_antennas in {16, 32, 64, 128, 256}, got " + std::to_string(N));
    if (M % N) return qce_set_error(QCE_ENOTIMPL, "observe_randsnr: features need M a multiple of n_antennas, got M = " +
                                                      std::to_string(M) + ", N = " + std::to_string(N));
    if (io == QCE_IO_DEVICE && ((uintptr_t)out & 15)) return qce_set_error(QCE_EARG, "observe_randsnr: feature output must be 16-byte aligned");
  }
  if (snr_index_in && io == QCE_IO_HOST)
    for (int64_t b = 0; b < B; ++b)
      if (snr_index_in[b] < 0 || snr_index_in[b] >= S) return qce_set_error(QCE_EARG, "observe_randsnr: SNR index out of range");
  if (B == 0) return QCE_OK;
  // A = kron(x, I_N), entry for entry: the kernel then keeps the one non-zero term of each row sum
  int P = 0;
  std::vector<double> xk;
  if (A && M % N == 0) {
    P = M / N;
    xk.resize(2 * (size_t)P);
    for (int p = 0; p < P; ++p) {
      xk[2 * p] = A[2 * ((size_t)p * N * N)];
      xk[2 * p + 1] = A[2 * ((size_t)p * N * N) + 1];
    }
    for (int m = 0; m < M && P; ++m)
      for (int c = 0; c < N; ++c) {
        const double re = A[2 * ((size_t)m * N + c)], im = A[2 * ((size_t)m * N + c) + 1];
        const bool diag = c == m % N;
        if (re != (diag ? xk[2 * (m / N)] : 0.0) || im != (diag ? xk[2 * (m / N) + 1] : 0.0)) {
          P = 0;
          break;
        }
      }
  }
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t ny = (size_t)B * M, nh = (size_t)B * N;
  const size_t out_bytes = out_kind == QCE_OUT_Y ? sizeof(double2) * ny : sizeof(float) * 2 * ny;
  const int nthr = kind == 1 ? n_levels - 1 : 0;
  QceObserveRowsArgs a;
  a.B = B;
  a.M = M;
  a.N = N;
  a.P = P;
  a.noise = noise_kind;
  a.seed = seed;
  a.row_offset = row_offset;
  a.S = S;
  a.kind = kind;
  a.nthr = nthr;
  a.out = out_kind;
  {
    StreamScratch sc(st);
    void* p;
    // one upload: scales, cdf, pilot vector, thresholds, labels
    const size_t n_thr = (size_t)S * nthr, n_lab = kind == 1 ? (size_t)S * n_levels : 0;
    std::vector<double> tab;
    tab.reserve(2 * (size_t)S + xk.size() + n_thr + n_lab);
    tab.insert(tab.end(), noise_scales, noise_scales + S);
    if (cdf) tab.insert(tab.end(), cdf, cdf + S);
    else tab.insert(tab.end(), (size_t)S, 0.0);
    if (P) tab.insert(tab.end(), xk.begin(), xk.end());
    if (kind == 1) {
      tab.insert(tab.end(), thresholds, thresholds + n_thr);
      tab.insert(tab.end(), labels, labels + n_lab);
    }
    HIPCHK(sc.get(&p, sizeof(double) * tab.size()));
    HIPCHK(hipMemcpyAsync(p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st));
    const double* dt = (const double*)p;
    a.scales = dt;
    a.cdf = cdf ? dt + S : nullptr;
    a.xk = P ? (const double2*)(dt + 2 * S) : nullptr;
    a.thr = kind == 1 ? dt + 2 * S + (P ? 2 * P : 0) : nullptr;
    a.lab = kind == 1 ? a.thr + n_thr : nullptr;
    a.A = nullptr;
    if (A && !P) {
      HIPCHK(sc.get(&p, sizeof(double2) * (size_t)M * N));
      HIPCHK(hipMemcpyAsync(p, A, sizeof(double2) * (size_t)M * N, hipMemcpyHostToDevice, st));
      a.A = (const double2*)p;
    }
    void* dout = out;
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&p, sizeof(double2) * nh));
      HIPCHK(hipMemcpyAsync(p, h, sizeof(double2) * nh, hipMemcpyHostToDevice, st));
      a.h = (const double2*)p;
      a.w = nullptr;
      if (noise_kind == 1) {
        HIPCHK(sc.get(&p, sizeof(double2) * ny));
        HIPCHK(hipMemcpyAsync(p, noise, sizeof(double2) * ny, hipMemcpyHostToDevice, st));
        a.w = (const double2*)p;
      }
      a.idx_in = nullptr;
      if (snr_index_in) {
        HIPCHK(sc.get(&p, sizeof(int) * (size_t)B));
        HIPCHK(hipMemcpyAsync(p, snr_index_in, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, st));
        a.idx_in = (const int*)p;
      }
      HIPCHK(sc.get(&p, sizeof(int) * (size_t)B));
      a.idx_out = (int*)p;
      HIPCHK(sc.get(&dout, out_bytes));
    } else {
      a.h = (const double2*)h;
      a.w = (const double2*)noise;
      a.idx_in = snr_index_in;
      a.idx_out = snr_index_out;
    }
    a.y = out_kind == QCE_OUT_Y ? (double2*)dout : nullptr;
    a.feat = out_kind == QCE_OUT_Y ? nullptr : (float*)dout;
    HIPCHK(qce_launch_observe_rows(a, st));
    if (io == QCE_IO_HOST) {
      HIPCHK(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(snr_index_out, a.idx_out, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    }
  }
  if (io == QCE_IO_HOST) HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_sq_error(const double* a, const double* b, int64_t n, double* out, int device, int io, void* stream) {
  if (n < 0 || !out || (n > 0 && (!a || !b))) return qce_set_error(QCE_EARG, "sq_error: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "sq_error: bad io");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  {
    StreamScratch sc(st);
    void *pa, *pb, *part, *po;
    HIPCHK(sc.get(&part, sizeof(double) * qce_sq_err_scratch()));
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&pa, sizeof(double2) * (size_t)n));
      HIPCHK(sc.get(&pb, sizeof(double2) * (size_t)n));
      HIPCHK(sc.get(&po, sizeof(double)));
      HIPCHK(hipMemcpyAsync(pa, a, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(pb, b, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, st));
    } else {
      pa = (void*)a;
      pb = (void*)b;
      po = out;
    }
    HIPCHK(qce_launch_sq_err(n, (const double2*)pa, (const double2*)pb, (double*)part, (double*)po, st));
    if (io == QCE_IO_HOST) HIPCHK(hipMemcpyAsync(out, po, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (io == QCE_IO_HOST) HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_em_estep(qce_model* m, const double* X, int64_t B, double* resp_out, double* mean_lse_out, int io,
                 void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 1 || !X || !resp_out || !mean_lse_out) return qce_set_error(QCE_EARG, "em_estep: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "em_estep: bad io");
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  const double2* dx = nullptr;
  if ((rc = stage_input(m, X, B, io, st, &dx))) return rc;
  const size_t BK = (size_t)B * m->K;
  HIPCHK(m->lp_scr.ensure(BK));
  double* dlp = m->lp_scr.p;
  if ((rc = backend_lp(m, dx, B, dlp, st))) return rc;
  {
    StreamScratch sc(st);
    void *lse, *part, *dresp = resp_out, *dmean = mean_lse_out;
    HIPCHK(sc.get(&lse, sizeof(double) * (size_t)B));
    HIPCHK(sc.get(&part, sizeof(double) * qce_mean_scratch()));
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&dresp, sizeof(double) * BK));
      HIPCHK(sc.get(&dmean, sizeof(double)));
    }
    HIPCHK(qce_launch_em_resp(B, m->K, dlp, (double*)dresp, (double*)lse, (double*)part, (double*)dmean, st));
    if (io == QCE_IO_HOST) {
      HIPCHK(hipMemcpyAsync(resp_out, dresp, sizeof(double) * BK, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(mean_lse_out, dmean, sizeof(double), hipMemcpyDeviceToHost, st));
    }
  }
  if (io == QCE_IO_HOST) HOST_SYNC_CHECK(m, st);
  return QCE_OK;
}

int qce_em_mstep(const double* X, int64_t B, int N, int K, const double* resp, double reg_covar, int diag,
                 int zero_mean, double* nk_out, double* means_out, double* covs_out, int device, int io,
                 void* stream) {
  if (B < 1 || N < 1 || N > 256 || K < 1 || !X || !resp || !nk_out || !means_out || !covs_out)
    return qce_set_error(QCE_EARG, "em_mstep: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "em_mstep: bad io");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  QceEmArgs a;
  a.B = B;
  a.N = N;
  a.K = K;
  a.diag = diag ? 1 : 0;
  a.zero_mean = zero_mean ? 1 : 0;
  a.reg = reg_covar;
  a.plan = qce_em_plan(B, N, K, a.diag);
  const size_t nX = (size_t)B * N, nR = (size_t)B * K, nM = (size_t)K * N;
  const size_t nC = a.diag ? nM : nM * N;
  const size_t cov_bytes = a.diag ? sizeof(double) * nC : sizeof(double2) * nC;
  {
    StreamScratch sc(st);
    void* p;
    HIPCHK(sc.get(&p, sizeof(double) * a.plan.stat_doubles));
    a.stats = (double*)p;
    a.part = nullptr;
    if (!a.diag) {
      HIPCHK(sc.get(&p, sizeof(double2) * a.plan.part_elems));
      a.part = (double2*)p;
    }
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&p, sizeof(double2) * nX));
      HIPCHK(hipMemcpyAsync(p, X, sizeof(double2) * nX, hipMemcpyHostToDevice, st));
      a.X = (const double2*)p;
      HIPCHK(sc.get(&p, sizeof(double) * nR));
      HIPCHK(hipMemcpyAsync(p, resp, sizeof(double) * nR, hipMemcpyHostToDevice, st));
      a.R = (const double*)p;
      HIPCHK(sc.get(&p, sizeof(double) * K));
      a.nk = (double*)p;
      HIPCHK(sc.get(&p, sizeof(double2) * nM));
      a.means = (double2*)p;
      HIPCHK(sc.get(&p, cov_bytes));
    } else {
      a.X = (const double2*)X;
      a.R = resp;
      a.nk = nk_out;
      a.means = (double2*)means_out;
      p = covs_out;
    }
    a.covs = a.diag ? nullptr : (double2*)p;
    a.diag_out = a.diag ? (double*)p : nullptr;
    HIPCHK(qce_launch_em_mstep(a, st));
    if (io == QCE_IO_HOST) {
      HIPCHK(hipMemcpyAsync(nk_out, a.nk, sizeof(double) * K, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(means_out, a.means, sizeof(double2) * nM, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(covs_out, p, cov_bytes, hipMemcpyDeviceToHost, st));
    }
  }
  if (io == QCE_IO_HOST) HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

static int assigned_impl(qce_model* m, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                         void* stream, int ls);

int qce_estimate_assigned(qce_model* m, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                          void* stream) {
  return assigned_impl(m, y, B, comp, h_out, io, stream, 0);
}

int qce_estimate_ls(qce_model* m, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                    void* stream) {
  return assigned_impl(m, y, B, comp, h_out, io, stream, 1);
}

int qce_estimate_ls_general(qce_model* m, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                            void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (m->M < m->N) return qce_set_error(QCE_ENOTIMPL, "general LS needs M >= N (full column rank A_eff)");
  return assigned_impl(m, y, B, comp, h_out, io, stream, 2);
}

static int assigned_impl(qce_model* m, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                         void* stream, int ls) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 0 || (B > 0 && (!y || !h_out))) return qce_set_error(QCE_EARG, "bad arguments");
  if (!comp && B > m->K) return qce_set_error(QCE_EARG, "without comp, sample b uses component b: B <= K");
  if (B == 0) return QCE_OK;
  if (m->backend == QCE_BE_BIG || m->M > 256)
    return qce_set_error(QCE_ENOTIMPL, "per-sample filters / LS cover N, M <= 256");
  if ((rc = ensure_dense(m))) return rc;
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  const double2* dy = nullptr;
  if ((rc = stage_input(m, y, B, io, st, &dy))) return rc;
  {
    StreamScratch sc(st);
    void* p;
    const long long* dc = reinterpret_cast<const long long*>(comp);
    double2* dh = reinterpret_cast<double2*>(h_out);
    if (comp && io == QCE_IO_HOST) {
      for (int64_t b = 0; b < B; ++b)
        if (comp[b] < 0 || comp[b] >= m->K) return qce_set_error(QCE_EARG, "component index out of range");
      HIPCHK(sc.get(&p, sizeof(long long) * (size_t)B));
      HIPCHK(hipMemcpyAsync(p, comp, sizeof(long long) * (size_t)B, hipMemcpyHostToDevice, st));
      dc = (const long long*)p;
    }
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&p, sizeof(double2) * (size_t)B * m->N));
      dh = (double2*)p;
    }
    if (ls == 2) {
      void *T, *P, *bz, *bad;
      HIPCHK(sc.get(&T, sizeof(double2) * (size_t)m->K * m->N * (m->N + m->M)));
      HIPCHK(sc.get(&P, sizeof(double2) * (size_t)m->K * m->N * m->M));
      HIPCHK(sc.get(&bz, sizeof(double2) * (size_t)m->K * m->N));
      HIPCHK(sc.get(&bad, sizeof(int) * (size_t)m->K));
      HIPCHK(qce_launch_ls_pinv(m->K, m->N, m->M, 0, m->Aeff.p, (double2*)T, (double2*)P, (double2*)bz, (int*)bad, st));
      std::vector<int> hb(m->K);
      HIPCHK(hipMemcpyAsync(hb.data(), bad, sizeof(int) * (size_t)m->K, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int k = 0; k < m->K; ++k)
        if (hb[k])
          return qce_set_error(QCE_ECHOL, "LS: A_eff of component " + std::to_string(k) +
                                     " is not of full column rank (Gram matrix pivot " + std::to_string(hb[k] - 1) +
                                     " vanishes)");
      HIPCHK(qce_launch_est_assigned(B, m->N, m->M, m->K, dy, dc, (const double2*)P, (const double2*)bz, dh, st));
    } else if (ls) HIPCHK(qce_launch_ls(B, m->N, m->M, dy, dc, m->Aeff.p, dh, st));
    else HIPCHK(qce_launch_est_assigned(B, m->N, m->M, m->K, dy, dc, m->W.p, m->bvec.p, dh, st));
    if (io == QCE_IO_HOST)
      HIPCHK(hipMemcpyAsync(h_out, dh, sizeof(double2) * (size_t)B * m->N, hipMemcpyDeviceToHost, st));
  }
  if (io == QCE_IO_HOST) HOST_SYNC_CHECK(m, st);
  return QCE_OK;
}

int qce_em_toeplitz(qce_model* m, const double* S, int K, int N, const double* F2, int P, double* sigma, double reg,
                    int init, double* covs_out, int device, void* stream) {
  if (!S || !F2 || !sigma || K < 1 || N < 1 || P < 1 || (!init && (!m || !covs_out)))
    return qce_set_error(QCE_EARG, "em_toeplitz: bad arguments");
  int rc;
  if (!init) {
    if ((rc = check_model(m, true))) return rc;
    if (m->K != K || m->N != N || m->M != N) return qce_set_error(QCE_EARG, "em_toeplitz: model shape mismatch");
    if ((rc = ensure_dense(m))) return rc;
    device = m->device;
  }
  DeviceGuard g(device);
  hipStream_t st = (!init && !stream) ? m->stream : (hipStream_t)stream;
  const size_t nn = (size_t)N * N, KNN = (size_t)K * nn;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0), mone = make_double2(-1.0, 0.0);
  {
    StreamScratch sc(st);
    void *dS, *dF, *dsg, *dG, *dC = nullptr, *dT = nullptr, *dM = nullptr;
    HIPCHK(sc.get(&dS, sizeof(double2) * KNN));
    HIPCHK(sc.get(&dF, sizeof(double2) * (size_t)P * N));
    HIPCHK(sc.get(&dsg, sizeof(double) * (size_t)K * P));
    HIPCHK(sc.get(&dG, sizeof(double2) * (size_t)K * P * N));
    HIPCHK(hipMemcpyAsync(dS, S, sizeof(double2) * KNN, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dF, F2, sizeof(double2) * (size_t)P * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsg, sigma, sizeof(double) * (size_t)K * P, hipMemcpyHostToDevice, st));
    const double2* Mx = (const double2*)dS;
    if (!init) {
      // Cinv = Linv^H Linv (the previous covariances' inverse, :808); Mx = Cinv S Cinv - Cinv (:812)
      HIPCHK(sc.get(&dC, sizeof(double2) * KNN));
      HIPCHK(sc.get(&dT, sizeof(double2) * KNN));
      HIPCHK(sc.get(&dM, sizeof(double2) * KNN));
      HIPCHK(qce_zgemm_batched(2, 0, N, N, N, one, m->Linv.p, N, nn, m->Linv.p, N, nn, zero, (double2*)dC, N, nn, K,
                               st));
      HIPCHK(qce_zgemm_batched(0, 0, N, N, N, one, (const double2*)dC, N, nn, (const double2*)dS, N, nn, zero,
                               (double2*)dT, N, nn, K, st));
      HIPCHK(hipMemcpyAsync(dM, dC, sizeof(double2) * KNN, hipMemcpyDeviceToDevice, st));
      HIPCHK(qce_zgemm_batched(0, 0, N, N, N, one, (const double2*)dT, N, nn, (const double2*)dC, N, nn, mone,
                               (double2*)dM, N, nn, K, st));
      Mx = (const double2*)dM;
    }
    // G_k = F2 Mx_k (P x N), then theta = Re diag(G_k F2^H)
    HIPCHK(qce_zgemm_batched(0, 0, P, N, N, one, (const double2*)dF, N, 0, Mx, N, nn, zero, (double2*)dG, N,
                             (long long)P * N, K, st));
    HIPCHK(qce_launch_inv_em_sigma(K, N, P, (const double2*)dG, (const double2*)dF, (double*)dsg, reg, init, st));
    HIPCHK(hipMemcpyAsync(sigma, dsg, sizeof(double) * (size_t)K * P, hipMemcpyDeviceToHost, st));
    if (!init) {
      HIPCHK(qce_launch_inv_em_cov(K, N, P, (const double2*)dF, (const double*)dsg, reg, (double2*)dT, st));
      HIPCHK(hipMemcpyAsync(covs_out, dT, sizeof(double2) * KNN, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_scm_generate(int64_t B, int n_coherence, int N, int n_path, double path_sigma, const double* gains,
                     const double* angles, const double* x, uint64_t seed, float* h_out, float* t_out, int device,
                     int io, void* stream) {
  if (B < 0 || n_coherence < 1 || N < 1 || N > 256 || n_path < 1 || n_path > qce_scm_max_path() ||
      (B > 0 && (!h_out || !t_out)) || (!gains) != (!angles))
    return qce_set_error(QCE_EARG, "scm_generate: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "scm_generate: bad io");
  if (B == 0) return QCE_OK;
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t F = 100 * (size_t)N, nh = (size_t)B * n_coherence * N, nt = (size_t)B * N;
  {
    StreamScratch sc(st);
    void* p;
    const double *dg = gains, *da = angles;
    const double2* dx = (const double2*)x;
    float2* dh = (float2*)h_out;
    float2* dt = (float2*)t_out;
    if (io == QCE_IO_HOST) {
      if (gains) {
        HIPCHK(sc.get(&p, sizeof(double) * 2 * (size_t)B * n_path));
        HIPCHK(hipMemcpyAsync(p, gains, sizeof(double) * (size_t)B * n_path, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((double*)p + (size_t)B * n_path, angles, sizeof(double) * (size_t)B * n_path,
                              hipMemcpyHostToDevice, st));
        dg = (const double*)p;
        da = (const double*)p + (size_t)B * n_path;
      }
      if (x) {
        HIPCHK(sc.get(&p, sizeof(double2) * (size_t)B * F * n_coherence));
        HIPCHK(hipMemcpyAsync(p, x, sizeof(double2) * (size_t)B * F * n_coherence, hipMemcpyHostToDevice, st));
        dx = (const double2*)p;
      }
      HIPCHK(sc.get(&p, sizeof(float2) * (nh + nt)));
      dh = (float2*)p;
      dt = (float2*)p + nh;
    }
    HIPCHK(qce_launch_scm(B, n_coherence, N, n_path, path_sigma, dg, da, dx, seed, dh, dt, st));
    if (io == QCE_IO_HOST) {
      HIPCHK(hipMemcpyAsync(h_out, dh, sizeof(float2) * nh, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(t_out, dt, sizeof(float2) * nt, hipMemcpyDeviceToHost, st));
    }
  }
  if (io == QCE_IO_HOST) HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_rate_bound(const double* h_est, const double* h, int64_t B, int N, const double* buss, const double* Cq,
                   double norm_clip, double* out, int device, int io, void* stream) {
  if (B < 1 || N < 1 || !h_est || !h || !buss || !Cq || !out) return qce_set_error(QCE_EARG, "rate_bound: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "rate_bound: bad io");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)B * N;
  {
    StreamScratch sc(st);
    void *dhe = (void*)h_est, *dh = (void*)h, *dbuss, *dcq, *inner, *den2, *part, *stat;
    HIPCHK(sc.get(&dbuss, sizeof(double) * N));
    HIPCHK(sc.get(&dcq, sizeof(double2) * (size_t)N * N));
    HIPCHK(hipMemcpyAsync(dbuss, buss, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dcq, Cq, sizeof(double2) * (size_t)N * N, hipMemcpyHostToDevice, st));
    HIPCHK(sc.get(&inner, sizeof(double2) * (size_t)B));
    HIPCHK(sc.get(&den2, sizeof(double) * (size_t)B));
    HIPCHK(sc.get(&part, sizeof(double) * qce_rate_scratch()));
    HIPCHK(sc.get(&stat, sizeof(double) * 8));
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&dhe, sizeof(double2) * nb));
      HIPCHK(sc.get(&dh, sizeof(double2) * nb));
      HIPCHK(hipMemcpyAsync(dhe, h_est, sizeof(double2) * nb, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(dh, h, sizeof(double2) * nb, hipMemcpyHostToDevice, st));
    }
    HIPCHK(qce_launch_rate(B, N, (const double2*)dhe, (const double2*)dh, (const double*)dbuss, (const double2*)dcq,
                           norm_clip, (double2*)inner, (double*)den2, (double*)part, (double*)stat, st));
    double res[6];
    HIPCHK(hipMemcpyAsync(res, stat, sizeof(double) * 6, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out[0] = res[5];  // rate
    out[1] = res[4];  // num
    out[2] = res[3];  // den1
    out[3] = res[2];  // den2
  }
  return QCE_OK;
}

int qce_rate_mf(const double* h_est, const double* h, int64_t B, int N, const double* buss, const double* Cq,
                double* out, int device, int io, void* stream) {
  if (B < 1 || N < 1 || N > 256 || !h_est || !h || !buss || !Cq || !out) return qce_set_error(QCE_EARG, "rate_mf: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "rate_mf: bad io");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)B * N, nn = (size_t)N * N;
  {
    StreamScratch sc(st);
    void *dhe = (void*)h_est, *dh = (void*)h, *dbuss, *dcq, *T, *cqi, *bz, *rate, *sum, *bad;
    HIPCHK(sc.get(&dbuss, sizeof(double) * N));
    HIPCHK(sc.get(&dcq, sizeof(double2) * nn));
    HIPCHK(sc.get(&T, sizeof(double2) * nn * 2));
    HIPCHK(sc.get(&cqi, sizeof(double2) * nn));
    HIPCHK(sc.get(&bz, sizeof(double2) * N));
    HIPCHK(sc.get(&rate, sizeof(double) * (size_t)B));
    HIPCHK(sc.get(&sum, sizeof(double)));
    HIPCHK(sc.get(&bad, sizeof(int)));
    HIPCHK(hipMemcpyAsync(dbuss, buss, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dcq, Cq, sizeof(double2) * nn, hipMemcpyHostToDevice, st));
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&dhe, sizeof(double2) * nb));
      HIPCHK(sc.get(&dh, sizeof(double2) * nb));
      HIPCHK(hipMemcpyAsync(dhe, h_est, sizeof(double2) * nb, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(dh, h, sizeof(double2) * nb, hipMemcpyHostToDevice, st));
    }
    HIPCHK(qce_launch_ls_pinv(1, N, N, 1, (const double2*)dcq, (double2*)T, (double2*)cqi, (double2*)bz, (int*)bad, st));
    HIPCHK(qce_launch_rate_mf(B, N, (const double2*)dhe, (const double2*)dh, (const double*)dbuss, (const double2*)dcq,
                              (const double2*)cqi, (double*)rate, (double*)sum, st));
    double r = 0.0;
    int hb = 0;
    HIPCHK(hipMemcpyAsync(&r, sum, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hb) return qce_set_error(QCE_ECHOL, "rate_mf: Cq is not positive definite (pivot " + std::to_string(hb - 1) + ")");
    out[0] = r / (double)B;
  }
  return QCE_OK;
}

int qce_vae_estimate(int N, int P, const double* x_cplx, double snr_db, double n_bits, const void* logvar,
                     int logvar_is_f32, const double* y, int64_t B, double* h_out, int io, int device, void* stream) {
  if (N < 1 || P < 1 || B < 0 || !x_cplx) return qce_set_error(QCE_EARG, "vae_estimate: bad shape");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "vae_estimate: bad io");
  if (B > 0 && (!logvar || !y || !h_out)) return qce_set_error(QCE_EARG, "vae_estimate: null buffer");
  if (N < 16 || N > 256 || (N & (N - 1)))
    return qce_set_error(QCE_ENOTIMPL, "vae_estimate: n_antennas must be a power of two in [16, 256], got " + std::to_string(N));
  if (P > QCE_VAE_MAX_PILOTS)
    return qce_set_error(QCE_ENOTIMPL, "vae_estimate: at most " + std::to_string(QCE_VAE_MAX_PILOTS) + " pilots, got " +
                                  std::to_string(P));
  QceVaeArgs a;
  if (int rc = vae_lmmse_args("vae_estimate", N, P, x_cplx, snr_db, n_bits, &a)) return rc;
  a.lv_f32 = logvar_is_f32 ? 1 : 0;
  if (B == 0) return QCE_OK;
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const size_t lvb = logvar_is_f32 ? sizeof(float) : sizeof(double);
  const int64_t CH = 1 << 16;  // samples per launch (and per staging buffer for host I/O)
  int status = 0;
  {
    StreamScratch sc(st);
    void *dstat, *dlv = nullptr, *dy = nullptr, *dh = nullptr;
    HIPCHK(sc.get(&dstat, sizeof(int)));
    HIPCHK(hipMemsetAsync(dstat, 0, sizeof(int), st));
    a.status = (int*)dstat;
    const int64_t cmax = B < CH ? B : CH;
    if (io == QCE_IO_HOST) {
      HIPCHK(sc.get(&dlv, lvb * (size_t)cmax * N));
      HIPCHK(sc.get(&dy, sizeof(double2) * (size_t)cmax * P * N));
      HIPCHK(sc.get(&dh, sizeof(double2) * (size_t)cmax * N));
    }
    for (int64_t b0 = 0; b0 < B; b0 += CH) {
      const int64_t nb = B - b0 < CH ? B - b0 : CH;
      const char* lv_c = (const char*)logvar + lvb * (size_t)b0 * N;
      const double* y_c = y + 2 * (size_t)b0 * P * N;
      double* h_c = h_out + 2 * (size_t)b0 * N;
      a.B = nb;
      if (io == QCE_IO_HOST) {
        HIPCHK(hipMemcpyAsync(dlv, lv_c, lvb * (size_t)nb * N, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dy, y_c, sizeof(double2) * (size_t)nb * P * N, hipMemcpyHostToDevice, st));
        a.lv = dlv;
        a.y = (const double2*)dy;
        a.h = (double2*)dh;
      } else {
        a.lv = lv_c;
        a.y = (const double2*)y_c;
        a.h = (double2*)h_c;
      }
      HIPCHK(qce_launch_vae(a, st));
      if (io == QCE_IO_HOST) HIPCHK(hipMemcpyAsync(h_c, dh, sizeof(double2) * (size_t)nb * N, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(&status, dstat, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (status)
    return qce_set_error(QCE_ECHOL, "vae_estimate: the quantised-observation covariance Cr is not positive definite in some "
                           "DFT bin (the reference's pinv has no counterpart here)");
  return QCE_OK;
}

}  // extern "C"
