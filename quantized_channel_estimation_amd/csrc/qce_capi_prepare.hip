// C ABI of libqce.so, per-SNR prepare: structure detection, the choice of the kernel family (select_backend), the
// Fourier-domain and dense table builds, and the Cholesky status a prepare posts for later calls to read.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "qce_capi.h"
#include "qce_common.h"

namespace {

int pad_dim(int v) {
  if (v <= 16) return 16;
  if (v <= 32) return 32;
  if (v <= 64) return 64;
  if (v <= 128) return 128;
  if (v <= 256) return 256;
  return -1;
}

bool fft_enabled() {
  const char* e = getenv("QCE_FFT");
  return !(e && e[0] == '0');
}

// QCE_FFT_KERNEL=lds keeps 'all' / partial on the LDS-tiled FP64 kernel of qce_fft.hip (A/B runs)
bool fft_mfma_enabled() {
  const char* e = getenv("QCE_FFT_KERNEL");
  return !(e && strcmp(e, "lds") == 0);
}

// A (M x N, interleaved complex) is the identity
bool is_identity(const double* A, int M, int N) {
  if (M != N) return false;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      const double re = A[2 * ((size_t)i * N + j)], im = A[2 * ((size_t)i * N + j) + 1];
      if (im != 0.0 || re != (i == j ? 1.0 : 0.0)) return false;
    }
  return true;
}

// A (M x N, interleaved complex) is exactly kron(x, I_N): M = P N, every off-diagonal entry of every N x N block is
// zero (+0 or -0: np.kron(x, I) yields -0 where x has a negative part, and either gives the same Cy) and the
// diagonal of block p is one value x_p.  Returns P and fills x for P <= 4 (the widest the Fourier family takes),
// 0 otherwise.
int pilot_vector(const double* A, int M, int N, double2* x) {
  if (!A || M % N != 0) return 0;
  const int P = M / N;
  if (P > 4) return 0;
  for (int p = 0; p < P; ++p) {
    const double* blk = A + 2 * (size_t)p * N * N;
    const double xr = blk[0], xi = blk[1];
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const double re = blk[2 * ((size_t)i * N + j)], im = blk[2 * ((size_t)i * N + j) + 1];
        if (i == j ? (re != xr || im != xi) : (re != 0.0 || im != 0.0)) return 0;
      }
    x[p] = make_double2(xr, xi);
  }
  return P;
}

// The one place a prepare's kernel family is chosen.  fourier_ok: the observation matrix is the identity and the
// call is not the dense replay of ensure_dense.  pilots: P when A = kron(x, I_N) with P <= 4 pilots (and the call is
// not that replay), else 0.  A dense family also gets its padded shape (MP, NP).
// int8_ok: the quantiser's outputs are integers up to 127 after one scale (1 bit, or uniform with 2..7 bits).
QceBackend select_backend(const qce_model* m, int M, bool fourier_ok, int pilots, bool int8_ok, int* MP, int* NP) {
  *MP = *NP = 0;
  if (fourier_ok && m->fft_n1 > 0 && fft_enabled() && !m->beta_first) return QCE_BE_FOURIER;
  if (m->fourier_pilots && pilots >= 2 && m->fft_n1 > 0 && fft_enabled() && !m->beta_first &&
      qce_fftp_shape(m->N, pilots, m->K))
    return QCE_BE_FOURIER_PILOTS;
  if (pad_dim(M) < 0 || pad_dim(m->N) < 0) return QCE_BE_BIG;
  *MP = pad_dim(M);
  *NP = pad_dim(m->N);
  if (*MP > 64 || *NP > 64) {  // the chunk-streamed kernel family (qce_estimate_h2x.hip) starts at 64
    *MP = *MP < 64 ? 64 : *MP;
    *NP = *NP < 64 ? 64 : *NP;
  }
  // the int8 family where it applies; everywhere else an int8 model takes the family it would take under f64
  if (want_int8(m) && int8_ok && qce_i8_shape(*MP, *NP)) return QCE_BE_INT8;
  if (want_f64(m) || want_int8(m)) {
    if (qce_f64_shape(*MP, *NP))  // the 3M layout where a 3M kernel covers the shape
      return qce_f64g_shape(*MP, *NP) ? QCE_BE_F64_3M : (qce_f64h_shape(*MP, *NP) ? QCE_BE_F64_3M_128 : QCE_BE_F64_4M);
    if (qce_wsum_shape(*MP, *NP)) return QCE_BE_F64_WIDE;
  }
  return QCE_BE_FAST;
}

// The Cholesky status of a prepare is copied to pinned host memory behind the prepare's kernels and read only
// when a call synchronises anyway (host I/O, qce_synchronize, qce_get_tables): a prepare costs no host round
// trip.  A failed prepare surfaces as QCE_ECHOL there (device-I/O estimates in between compute on NaN tables).
int post_status(qce_model* m, hipStream_t st) {
  const int K = m->K;
  if (!m->status_host) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&m->status_host), sizeof(int) * K, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&m->status_ev, hipEventDisableTiming));
  }
  HIPCHK(hipMemcpyAsync(m->status_host, m->status.p, sizeof(int) * K, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(m->status_ev, st));
  m->status_pending = 1;
  return QCE_OK;
}

}  // namespace

// Is every C_k (block-)circulant for some power-of-two split N = n1 n2?  (circulant fit:
// gmm_cplx_bussgang.py:104-117, block-circulant fit: :118-133).  Sets fft_n1/fft_n2 and keeps the
// eigenvalues, first columns and mean spectra for the per-SNR Fourier prepare.
hipError_t detect_structure(qce_model* m) {
  const int K = m->K, N = m->N;
  m->fft_n1 = m->fft_n2 = 0;
  if (N > 256 || !qce_fft_pow2(N) || N < 4 || qce_fft_tile(N, K) == 0 || K > 256) return hipSuccess;
  hipError_t e;
  if ((e = m->f_ceig.ensure((size_t)K * N)) != hipSuccess) return e;
  if ((e = m->f_col0.ensure((size_t)K * N)) != hipSuccess) return e;
  if ((e = m->f_mspec.ensure((size_t)K * N)) != hipSuccess) return e;
  if ((e = m->f_bad.ensure(K)) != hipSuccess) return e;
  std::vector<int> bad(K);
  for (int n1 = 1; n1 < N; n1 *= 2) {
    const int n2 = N / n1;
    if ((e = qce_launch_fft_struct(K, N, n1, n2, 1e-10, m->covs.p, m->means.p, m->f_ceig.p, m->f_col0.p,
                                   m->f_mspec.p, m->f_bad.p, m->stream)) != hipSuccess)
      return e;
    if ((e = hipMemcpyAsync(bad.data(), m->f_bad.p, sizeof(int) * K, hipMemcpyDeviceToHost, m->stream)) != hipSuccess)
      return e;
    if ((e = hipStreamSynchronize(m->stream)) != hipSuccess) return e;
    bool ok = true;
    for (int k = 0; k < K; ++k) ok = ok && bad[k] == 0;
    if (ok) {
      m->fft_n1 = n1;
      m->fft_n2 = n2;
      return hipSuccess;
    }
  }
  m->f_ceig.release();
  m->f_col0.release();
  m->f_mspec.release();
  return hipSuccess;
}

// Uniform quantiser step get_uniform_quant_step (uniform_quantizer.py:44-45) with standard_quantization_step
// (:6-23): J. Max's table for n_bits <= 8, the asymptote 4 sqrt(b) 2^-b of Hui & Neuhoff beyond it (:15-21).
double uniform_std_step(int nb) {
  static const double tbl[9] = {0, 1.596, 0.9957, 0.5860, 0.3352, 0.1881, 0.1041, 0.0569, 0.0308};
  return nb <= 8 ? tbl[nb] : 4.0 * sqrt((double)nb) * pow(2.0, -nb);
}

double uniform_step(double snr_db, int nb) {
  return sqrt((1.0 + pow(10.0, -snr_db / 10.0)) / 2.0) * uniform_std_step(nb);
}

int check_status(qce_model* m, bool block) {
  if (!m->status_pending) return QCE_OK;
  if (!block && hipEventQuery(m->status_ev) == hipErrorNotReady) return QCE_OK;
  HIPCHK(hipEventSynchronize(m->status_ev));
  m->status_pending = 0;
  for (int k = 0; k < m->K; ++k)
    if (m->status_host[k]) {
      m->prepared = 0;
      return qce_set_error(QCE_ECHOL,
                  "Fitting the mixture model failed because some components have ill-defined empirical covariance "
                  "(for instance caused by singleton or collapsed samples). Try to decrease the number of "
                  "components, or increase reg_covar.");
    }
  return QCE_OK;
}

int check_model(qce_model* m, bool need_prepared) {
  if (!m) return qce_set_error(QCE_EARG, "null model");
  if (need_prepared && m->prepared)
    if (int rc = check_status(m, false)) return rc;  // a failure already known surfaces at once
  if (need_prepared && !m->prepared) return qce_set_error(QCE_ESTATE, "qce_prepare has not been called on this model");
  return QCE_OK;
}

// tables_only: the dense replay of ensure_dense (the Fourier tables stay the active family)
static int prepare_impl(qce_model* m, const double* A, int M, double snr_db, double n_bits, int quant_kind,
                        const double* thresholds, const double* labels, int n_levels, void* stream,
                        bool tables_only) {
  int rc = check_model(m, false);
  if (rc) return rc;
  const int N = m->N, K = m->K;
  if (!A) M = N;
  if (M <= 0) return qce_set_error(QCE_EARG, "M must be positive");
  if (M > QCE_BIG_MAX) return qce_set_error(QCE_ENOTIMPL, "M > " + std::to_string(QCE_BIG_MAX) + " is not covered");
  int kind;
  int nb = 0;
  if (n_bits == 1.0) {
    kind = 0;
  } else if (isinf(n_bits) && n_bits > 0) {
    kind = 2;
  } else {
    if (!(n_bits >= 2.0 && n_bits <= (double)QCE_MAX_UNIFORM_BITS) || n_bits != floor(n_bits))
      return qce_set_error(QCE_ENOTIMPL, "n_bits must be 1.." + std::to_string(QCE_MAX_UNIFORM_BITS) + " or inf");
    kind = 1;
    nb = (int)n_bits;
    if (quant_kind == QCE_QUANT_LLOYD && nb > 8)
      return qce_set_error(QCE_ENOTIMPL, "lloyd quantiser tables cover n_bits <= 8");
  }
  if (kind == 1 && quant_kind == QCE_QUANT_LLOYD) {
    if (!thresholds || !labels || n_levels != (1 << nb))
      return qce_set_error(QCE_EARG, "lloyd quantiser needs 2^b labels and 2^b-1 thresholds");
  }
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  // an explicit identity is the same observation model (and takes the same fast path: bitwise the same Cy)
  const bool idA = !A || is_identity(A, M, N);
  int MP, NP;
  const bool int8_ok = kind == 0 || (kind == 1 && quant_kind == QCE_QUANT_UNIFORM && nb >= 2 && nb <= 7);
  double2 px[4] = {};
  const int pilots = (!idA && !tables_only && m->fourier_pilots) ? pilot_vector(A, M, N, px) : 0;
  const QceBackend be = select_backend(m, M, idA && !tables_only, pilots, int8_ok, &MP, &NP);
  m->last.M = M;
  m->last.snr_db = snr_db;
  m->last.n_bits = n_bits;
  m->last.quant_kind = quant_kind;
  m->last.n_levels = n_levels;
  if (!tables_only) {
    m->last.thr.assign(thresholds && kind == 1 ? thresholds : nullptr,
                       thresholds && kind == 1 ? thresholds + (n_levels > 0 ? n_levels - 1 : 0) : nullptr);
    m->last.lab.assign(labels && kind == 1 ? labels : nullptr, labels && kind == 1 ? labels + n_levels : nullptr);
  }
  // both table builds: the status words, and the quantiser's step or Lloyd tables
  HIPCHK(m->status.ensure(K));
  HIPCHK(m->thr.ensure(256));
  HIPCHK(m->lab.ensure(256));
  double delta = 0.0;
  if (kind == 1 && quant_kind == QCE_QUANT_UNIFORM) delta = uniform_step(snr_db, nb);
  if (kind == 1 && quant_kind == QCE_QUANT_LLOYD) {
    HIPCHK(hipMemcpyAsync(m->thr.p, thresholds, sizeof(double) * (n_levels - 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(m->lab.p, labels, sizeof(double) * n_levels, hipMemcpyHostToDevice, st));
  }
  if (be == QCE_BE_FOURIER) {
    // Fourier-domain prepare (qce_fft.hip): per-bin tables only
    HIPCHK(m->f_rinvT.ensure((size_t)N * K));
    HIPCHK(m->f_uT.ensure((size_t)N * K));
    HIPCHK(m->f_cprime.ensure(K));
    HIPCHK(m->f_wT.ensure((size_t)K * N));
    HIPCHK(m->f_bT.ensure((size_t)K * N));
    HIPCHK(m->f_gain.ensure(K));
    QceFftPrepArgs fa;
    fa.N = N;
    fa.n1 = m->fft_n1;
    fa.n2 = m->fft_n2;
    fa.K = K;
    fa.s2 = pow(10.0, -snr_db / 10.0);
    fa.kind = kind;
    fa.n_bits = nb;
    fa.quant_kind = quant_kind;
    fa.delta = delta;
    fa.thr = m->thr.p;
    fa.lab = m->lab.p;
    fa.logw = m->logw.p;
    fa.ceig = m->f_ceig.p;
    fa.col0 = m->f_col0.p;
    fa.mspec = m->f_mspec.p;
    fa.rinvT = m->f_rinvT.p;
    fa.uT = m->f_uT.p;
    fa.cprime = m->f_cprime.p;
    fa.wT = m->f_wT.p;
    fa.bT = m->f_bT.p;
    fa.gain = m->f_gain.p;
    fa.status = m->status.p;
    HIPCHK(qce_launch_fft_prep(fa, st));
    m->fft_mfma = 0;
    if (qce_fft_mfma_shape(N) && fft_mfma_enabled()) {
      const size_t KpN = (size_t)qce_fft_kpad(K) * N;
      HIPCHK(m->f_pr.ensure(KpN));
      HIPCHK(m->f_pc.ensure((size_t)qce_fft_kpad(K)));
      HIPCHK(m->f_pw.ensure(KpN));
      if (m->has_mean) {
        HIPCHK(m->f_pur.ensure(KpN));
        HIPCHK(m->f_pui.ensure(KpN));
        HIPCHK(m->f_pbr.ensure(KpN));
        HIPCHK(m->f_pbi.ensure(KpN));
      }
      QceFftEstArgs pa = fft_args(m, nullptr, 0);
      HIPCHK(qce_launch_fft_pack(pa, m->f_rinvT.p, m->f_uT.p, m->f_cprime.p, m->f_wT.p, m->f_bT.p, st));
      m->fft_mfma = 1;
    }
    if ((rc = post_status(m, st))) return rc;
    m->M = N;
    m->backend = be;
    m->dense_valid = 0;
    m->prepared = 1;
    return QCE_OK;
  }
  if (be == QCE_BE_FOURIER_PILOTS) {
    // Fourier-domain prepare with pilots (qce_fft_pilot.hip): per-bin P x P tables only; A is kept for the dense replay
    const int Kp = qce_fftp_kpad(K);
    m->last.A.assign(A, A + 2 * (size_t)M * N);
    HIPCHK(m->fp_tabL.ensure((size_t)qce_fftp_tabl_doubles(N, pilots, Kp, m->has_mean)));
    HIPCHK(m->fp_tabW.ensure((size_t)qce_fftp_tabw_doubles(N, pilots, Kp, m->has_mean)));
    HIPCHK(m->fp_cprime.ensure((size_t)Kp));
    QceFftpPrepArgs fa;
    fa.N = N;
    fa.n1 = m->fft_n1;
    fa.n2 = m->fft_n2;
    fa.K = K;
    fa.Kp = Kp;
    fa.P = pilots;
    fa.has_mean = m->has_mean;
    for (int p = 0; p < 4; ++p) fa.x[p] = m->fp_x[p] = px[p];
    fa.s2 = pow(10.0, -snr_db / 10.0);
    fa.kind = kind;
    fa.n_bits = nb;
    fa.quant_kind = quant_kind;
    fa.delta = delta;
    fa.thr = m->thr.p;
    fa.lab = m->lab.p;
    fa.logw = m->logw.p;
    fa.ceig = m->f_ceig.p;
    fa.col0 = m->f_col0.p;
    fa.mspec = m->f_mspec.p;
    fa.tabL = m->fp_tabL.p;
    fa.cprime = m->fp_cprime.p;
    fa.tabW = m->fp_tabW.p;
    fa.status = m->status.p;
    HIPCHK(qce_launch_fftp_prep(fa, st));
    if ((rc = post_status(m, st))) return rc;
    m->fp_P = pilots;
    m->M = M;
    m->backend = be;
    m->dense_valid = 0;
    m->prepared = 1;
    return QCE_OK;
  }
  if (!tables_only) m->backend = be;
  m->dense_valid = 1;
  const size_t KMM = (size_t)K * M * M, KMN = (size_t)K * M * N;
  HIPCHK(m->A.ensure((size_t)M * N));
  HIPCHK(m->Cy.ensure(KMM));
  HIPCHK(m->Cr.ensure(KMM));
  HIPCHK(m->Lw.ensure(KMM));
  HIPCHK(m->Linv.ensure(KMM));
  HIPCHK(m->Aeff.ensure(KMN));
  HIPCHK(m->work.ensure(KMN));
  HIPCHK(m->V.ensure(KMN));
  HIPCHK(m->W.ensure(KMN));
  HIPCHK(m->means_y.ensure((size_t)K * M));
  // a buffer about to be reallocated holds no zeros yet (and keeps none if its allocation fails)
  if (m->q0.n < (size_t)K * M) m->q0_zeroed = 0;
  if (m->bvec.n < (size_t)K * N) m->bvec_zeroed = 0;
  HIPCHK(m->q0.ensure((size_t)K * M));
  HIPCHK(m->bvec.ensure((size_t)K * N));
  if (m->has_mean) {
    m->q0_zeroed = m->bvec_zeroed = 0;  // the prepare writes them
  } else if (m->q0_zeroed < (size_t)K * M || m->bvec_zeroed < (size_t)K * N) {  // zero-mean: q0 = 0, b = 0 at every SNR
    m->q0_zeroed = m->bvec_zeroed = 0;
    HIPCHK(hipMemsetAsync(m->q0.p, 0, sizeof(double2) * m->q0.n, st));
    HIPCHK(hipMemsetAsync(m->bvec.p, 0, sizeof(double2) * m->bvec.n, st));
    m->q0_zeroed = m->q0.n;
    m->bvec_zeroed = m->bvec.n;
  }
  HIPCHK(m->gain.ensure((size_t)K * M));
  HIPCHK(m->cconst.ensure(K));
  m->big_ws_valid = 0;
  const bool big = be == QCE_BE_BIG;
  const long long s32 = big ? 0 : qce_pack_f32_stride(MP, NP, m->has_mean);
  const long long s64 = big ? 0 : qce_pack_f64_stride(MP, m->has_mean);
  HIPCHK(m->pack32.ensure((size_t)s32 * K));
  HIPCHK(m->pack64.ensure((size_t)s64 * K));
  if (A) {
    HIPCHK(hipMemcpyAsync(m->A.p, A, sizeof(double2) * (size_t)M * N, hipMemcpyHostToDevice, st));
    m->a_identity_n = 0;
  } else if (m->a_identity_n != N) {
    std::vector<double> eye((size_t)2 * N * N, 0.0);
    for (int i = 0; i < N; ++i) eye[(size_t)2 * (i * N + i)] = 1.0;
    HIPCHK(hipMemcpyAsync(m->A.p, eye.data(), sizeof(double2) * (size_t)N * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    m->a_identity_n = N;
  }
  QcePrepareArgs p;
  p.K = K;
  p.N = N;
  p.M = M;
  p.MP = MP;
  p.NP = NP;
  p.has_mean = m->has_mean;
  p.identityA = idA;
  p.kind = kind;
  p.n_bits = nb;
  p.quant_kind = quant_kind;
  p.beta_first = m->beta_first;
  p.sigma2 = pow(10.0, -snr_db / 10.0);
  p.delta = delta;
  p.thr = m->thr.p;
  p.lab = m->lab.p;
  p.A = m->A.p;
  p.covs = m->covs.p;
  p.means = m->means.p;
  p.logw = m->logw.p;
  p.Cy = m->Cy.p;
  p.Cr = m->Cr.p;
  p.Lw = m->Lw.p;
  p.Linv = m->Linv.p;
  p.Aeff = m->Aeff.p;
  p.work = m->work.p;
  p.V = m->V.p;
  p.W = m->W.p;
  p.means_y = m->means_y.p;
  p.q0 = m->q0.p;
  p.bvec = m->bvec.p;
  p.gain = m->gain.p;
  p.cconst = m->cconst.p;
  p.status = m->status.p;
  p.pack32 = m->pack32.p;
  p.stride32 = s32;
  p.pack64 = m->pack64.p;
  p.stride64 = s64;
  m->pack_args = p;
  m->packs_valid = 0;
  m->pack64_valid = 0;
  m->wt_valid = 0;
  p.pack32 = nullptr;  // selective-mode / log-prob tables are packed on first use (ensure_packs)
  p.pack64 = nullptr;
  HIPCHK(qce_launch_prepare(p, st));
  switch (be) {
    case QCE_BE_NONE:
    case QCE_BE_FOURIER:  // returned above
    case QCE_BE_FOURIER_PILOTS:
    case QCE_BE_BIG:
      // GEMM-based FP64 path (qce_big.hip): the dense tables are all it reads; the stacked filters on first use
      break;
    case QCE_BE_F64_WIDE:
      // FP64 filter tables of the two-pass path; the log-prob table is packed on first use (ensure_pack64)
      HIPCHK(m->pack_ws.ensure((size_t)qce_pack_wsum_bytes(MP, NP, m->has_mean) * K));
      HIPCHK(qce_launch_pack_wsum(K, M, N, MP, NP, m->has_mean, m->W.p, m->bvec.p,
                                  reinterpret_cast<double*>(m->pack_ws.p), st));
      break;
    // FP64 tables of the fused kernels (reference precision)
    case QCE_BE_F64_3M_128:
      HIPCHK(m->pack_f64.ensure((size_t)qce_pack_f64h_bytes(m->has_mean) * K));
      HIPCHK(qce_launch_pack_f64h(K, M, N, m->has_mean, m->Linv.p, m->W.p, m->q0.p, m->bvec.p,
                                  reinterpret_cast<double*>(m->pack_f64.p), st));
      break;
    case QCE_BE_F64_3M:
      HIPCHK(m->pack_f64.ensure((size_t)qce_pack_f64g_bytes(MP, NP, m->has_mean) * K));
      HIPCHK(qce_launch_pack_f64g(K, M, N, MP, NP, m->has_mean, m->Linv.p, m->W.p, m->q0.p, m->bvec.p,
                                  reinterpret_cast<double*>(m->pack_f64.p), st));
      break;
    case QCE_BE_F64_4M:
      HIPCHK(m->pack_f64.ensure((size_t)qce_pack_f64all_bytes(MP, NP, m->has_mean) * K));
      HIPCHK(qce_launch_pack_f64all(K, M, N, MP, NP, m->has_mean, m->Linv.p, m->W.p, m->q0.p, m->bvec.p,
                                    reinterpret_cast<double*>(m->pack_f64.p), st));
      break;
    case QCE_BE_INT8: {
      // digit planes of E(Linv_k), E(W_k); the observation scale that makes the quantiser outputs integers
      const double y_scale = kind == 0 ? sqrt(2.0) : 2.0 / delta;
      const int S = m->int8_slices;
      HIPCHK(m->i8_planes.ensure((size_t)qce_pack_i8_bytes(MP, NP, S) * K));
      HIPCHK(m->i8_rowtab.ensure((size_t)(4 * MP + 4 * NP) * K));
      HIPCHK(m->i8_exps.ensure((size_t)(2 * MP + 2 * NP) * K));
      HIPCHK(qce_launch_pack_i8(K, M, N, MP, NP, S, y_scale, m->Linv.p, m->W.p, m->q0.p, m->bvec.p, m->i8_planes.p,
                                m->i8_rowtab.p, m->i8_exps.p, st));
      m->i8_S = S;
      m->i8_group = kind == 0 ? 3 : 2;
      m->y_scale = y_scale;
      break;
    }
    case QCE_BE_FAST: {
      // FP16 two-term split tables; the observation scale makes quantiser outputs exact in fp16
      // (1 bit: y sqrt(2) = +-1; uniform: y 2/delta = odd integers), folded into the slice scales
      double y_scale = 1.0;
      if (kind == 0) y_scale = sqrt(2.0);
      else if (kind == 1 && quant_kind == QCE_QUANT_UNIFORM && delta > 0.0) y_scale = 2.0 / delta;
      const long long cs16 = qce_pack_h2_stride_bytes(MP, NP, m->has_mean);
      const int nslices = (2 * MP) / 32 + (2 * NP) / 32;
      HIPCHK(m->pack16.ensure((size_t)cs16 * K + (size_t)qce_h2x_pad_bytes()));
      HIPCHK(m->sinv.ensure((size_t)nslices * K));
      HIPCHK(qce_launch_pack_h2(K, M, N, MP, NP, m->has_mean, cs16, y_scale, m->Linv.p, m->W.p, m->q0.p, m->bvec.p,
                                m->pack16.p, m->sinv.p, st));
      m->cstride16 = cs16;
      m->y_scale = y_scale;
      break;
    }
  }
  if ((rc = post_status(m, st))) return rc;
  m->M = M;
  m->MP = MP;
  m->NP = NP;
  m->stride32 = s32;
  m->stride64 = s64;
  m->prepared = 1;
  return QCE_OK;
}

// The dense tables of a prepare that took the Fourier path, computed when first asked for
// (qce_get_tables: the reference's gm state mirror); the Fourier tables stay active.
int ensure_dense(qce_model* m, void* stream) {
  if (!qce_be_fourier(m->backend) || m->dense_valid) return QCE_OK;
  // the pilots family replays with the A it was prepared with (kept on the host)
  const double* A = m->backend == QCE_BE_FOURIER_PILOTS ? m->last.A.data() : nullptr;
  return prepare_impl(m, A, m->last.M, m->last.snr_db, m->last.n_bits, m->last.quant_kind,
                      m->last.thr.empty() ? nullptr : m->last.thr.data(),
                      m->last.lab.empty() ? nullptr : m->last.lab.data(), m->last.n_levels, stream, true);
}

extern "C" int qce_prepare(qce_model* m, const double* A, int M, double snr_db, double n_bits, int quant_kind,
                           const double* thresholds, const double* labels, int n_levels, void* stream) {
  return prepare_impl(m, A, M, snr_db, n_bits, quant_kind, thresholds, labels, n_levels, stream, false);
}
