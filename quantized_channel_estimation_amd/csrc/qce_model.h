// Private layout of a qce_model (the opaque handle of include/qce.h), shared by the C-ABI units
// (qce_capi*.hip: model lifetime / prepare / estimate; qce_kshard.hip: the K-shard step over a communicator).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "qce_kernels.h"

// A device buffer that owns its memory.  Only ever a member of a handle (qce_model, qce_kshard) that an explicit
// destroy call deletes under the device guard while the HIP runtime is up: never static or thread-local, so no
// hipFree runs at process exit.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(&p, sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// The kernel family that serves 'all' / partial / log-prob calls of a prepared model.  Chosen in one place
// (select_backend, qce_capi_prepare.hip) and switched on by every entry point.
enum QceBackend {
  QCE_BE_NONE = 0,     // not prepared
  QCE_BE_FOURIER,      // (block-)circulant mixture, Fourier-domain tables (qce_fft.hip / qce_fft_mfma.hip)
  QCE_BE_BIG,          // N or M beyond 256: GEMM-based FP64 path (qce_big.hip)
  QCE_BE_F64_4M,       // fused FP64 kernel k_est_all_f64
  QCE_BE_F64_3M,       // 3M layout, padded <= 64 (k_est_all_f64g)
  QCE_BE_F64_3M_128,   // 3M layout at padded 128 (k_est_all_f64h)
  QCE_BE_F64_WIDE,     // beyond padded 128: the two-pass FP64 path (qce_wsum_f64.hip)
  QCE_BE_FAST,         // fp16-split / FP32-MFMA kernels (QCE_KERNEL picks between them per launch)
  QCE_BE_INT8,         // int8 digit planes on the i8 MFMA, quantised observations, padded <= 64 (k_est_all_i8)
  QCE_BE_FOURIER_PILOTS,  // (block-)circulant mixture, A = kron(x, I_N): per-bin P x P tables (qce_fft_pilot.hip)
};
// the Fourier-domain families: per-bin tables are the active ones, the dense tables are computed on demand
inline bool qce_be_fourier(QceBackend be) { return be == QCE_BE_FOURIER || be == QCE_BE_FOURIER_PILOTS; }

struct qce_model {
  int K = 0, N = 0, device = 0;
  int a_identity_n = 0;   // m->A holds I_N (skips the upload + sync of a repeated A = NULL prepare)
  // zero-mean model: the first q0_zeroed / bvec_zeroed elements of q0 / bvec hold zeros (the prepare then skips
  // their three launches).  Counted in elements, not remembered by address: a DevBuf::ensure that grows
  // the buffer may get the old address back from hipMalloc, and the grown tail must be zeroed again
  size_t q0_zeroed = 0, bvec_zeroed = 0;
  int packs_valid = 0;    // pack32 / pack64 built for the current prepare (lazy: 'all' mode never needs them)
  QcePrepareArgs pack_args{};
  int beta_first = 0;  // QCE_OPT_BETA_FIRST: multi-bit Cr mixes with the first gain (blmmse.py:53, :86)
  int precision = QCE_PRECISION_F64;  // QCE_OPT_PRECISION: arithmetic of the dense 'all' / partial path
  int int8_slices = 7;  // QCE_OPT_INT8_SLICES: digit planes per table under QCE_PRECISION_INT8
  int fourier_pilots = 0;  // QCE_OPT_FOURIER_PILOTS: A = kron(x, I_N) on a structured model takes the Fourier family
  hipStream_t stream = nullptr;
  int has_mean = 0;
  std::vector<double> weights;
  DevBuf<double2> means, covs;
  DevBuf<double> logw;
  // prepared state
  int M = 0, MP = 0, NP = 0, prepared = 0;
  // Family of the last prepare.  A Fourier prepare leaves the dense tables (and MP / NP) of an earlier prepare
  // behind; dense_valid says whether they match this prepare (ensure_dense replays it without touching `backend`).
  QceBackend backend = QCE_BE_NONE;
  DevBuf<double2> A, Cy, Cr, Lw, Linv, Aeff, work, V, W, means_y, q0, bvec;
  DevBuf<double> gain, cconst, thr, lab;
  DevBuf<int> status;
  int* status_host = nullptr;  // pinned copy of the last prepare's Cholesky status (read lazily)
  hipEvent_t status_ev = nullptr;
  int status_pending = 0;
  DevBuf<float> pack32;
  DevBuf<double> pack64;
  long long stride32 = 0, stride64 = 0;
  // estimate scratch
  DevBuf<double2> y_scr, h_scr;
  DevBuf<double> lp_scr, proba_scr, m_scr, s_scr;
  DevBuf<float> w_scr, acc_scr;
  DevBuf<long long> lab_scr;
  // FP16 two-term split tables (qce_estimate_h2.hip)
  DevBuf<char> pack16;
  DevBuf<float> sinv;
  long long cstride16 = 0;
  double y_scale = 1.0;
  DevBuf<double> sp_m, sp_s;
  DevBuf<float> sp_a;
  DevBuf<int> yflag;
  // int8 digit planes, row tables and row exponents (qce_estimate_i8.hip); i8_group: planes combined in int32
  DevBuf<signed char> i8_planes;
  DevBuf<double> i8_rowtab;
  DevBuf<int> i8_exps;
  int i8_S = 0, i8_group = 2;
  // FP64 fused-kernel tables (qce_estimate_f64.hip) and its cut-tile scratch
  DevBuf<char> pack_f64;
  DevBuf<char> pack_ws;  // ... and of the two-pass path (qce_wsum_f64.hip)
  int pack64_valid = 0;  // pack64 (the k_lp_f64 table) built without pack32
  DevBuf<double> fp_m, fp_s, fp_a;
  DevBuf<double> fp_scr;    // two-pass 3M kernel: softmax weights, K x 128 per workgroup of the launch
  DevBuf<double> part_a64;  // FP64 partial accumulator behind the f32 qce_estimate_partial
  DevBuf<double> fp_pack;   // host-I/O staging of qce_estimate_partial_shifted
  DevBuf<double> w64_scr;   // FP64 selection weights (selective modes)
  DevBuf<double> shift_scr;  // one double: staged K-shard shift / cconst max
  DevBuf<double2> WT;       // transposed filters W_k^T for the FP64 selective-mode kernel (built lazily)
  int wt_valid = 0;
  int cu_count = 256;
  int reserve_cus = 0;  // QCE_OPT_RESERVE_CUS: CUs the persistent grids leave to a concurrent communication stream
  int reserve_set = 0;  // the caller set QCE_OPT_RESERVE_CUS (a K-shard step then keeps the caller's value)
  int sched_cus() const { return cu_count - reserve_cus > 8 ? cu_count - reserve_cus : 8; }
  // dimensions beyond the fused kernels' 256 (qce_big.hip): GEMM-based FP64 path
  DevBuf<double2> big_ws, big_d;  // stacked transposed filters (N x K x M); per-chunk intermediate
  int big_ws_valid = 0;
  // Fourier-domain path for (block-)circulant mixtures (qce_fft.hip): structure found at creation
  int fft_n1 = 0, fft_n2 = 0;
  int dense_valid = 0;  // dense tables match the last prepare (after a Fourier prepare: computed lazily)
  DevBuf<double> f_ceig, f_rinvT, f_cprime, f_wT, f_gain;
  DevBuf<double2> f_col0, f_mspec, f_uT, f_bT;
  DevBuf<int> f_bad;
  DevBuf<double> f_pr, f_pur, f_pui, f_pc, f_pw, f_pbr, f_pbi;  // qce_fft_mfma.hip tables
  int fft_mfma = 0;                                            // the MFMA kernel serves 'all' / partial
  // ... with pilots, A = kron(x, I_N) (qce_fft_pilot.hip): pilot count and vector of the last such prepare, tables
  int fp_P = 0;
  double2 fp_x[4] = {};
  DevBuf<double> fp_tabL, fp_tabW, fp_cprime;
  // host-I/O pipeline of qce_estimate: two pinned slots per direction, copy-in / copy-out streams
  struct {
    double2* pin_y[2] = {nullptr, nullptr};
    double2* pin_h[2] = {nullptr, nullptr};
    size_t cap_y = 0, cap_h = 0;  // elements per slot
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  } hp;
  // arguments of the last prepare (replayed for the dense tables qce_get_tables returns)
  struct {
    int M = 0, quant_kind = 0, n_levels = 0;
    double snr_db = 0.0, n_bits = 1.0;
    std::vector<double> thr, lab;
    std::vector<double> A;  // the observation matrix of a prepare onto QCE_BE_FOURIER_PILOTS (interleaved complex)
  } last;
};

// Internal entry point of qce_capi_estimate.hip used by qce_kshard.hip (C++ linkage: not part of the ABI).
// h_b = sum_k w[b][k] (W_k y_b + b_k), w (B x K) FP64 selection weights on the device (dense or Fourier path)
int qce_weighted_estimate(qce_model* m, const double2* y, long long B, const double* w, double2* h, hipStream_t st);

// qce_big.hip: the GEMM-based FP64 path for N or M in (256, QCE_BIG_MAX]
#define QCE_BIG_MAX 4096
int qce_big_lp(qce_model* m, const double2* y, long long B, double* lp, hipStream_t st);
int qce_big_proba(qce_model* m, long long B, hipStream_t st);
int qce_big_wsum(qce_model* m, const double2* y, long long B, const double* w, double2* out, long long ldo,
                 hipStream_t st);
int qce_big_partial(qce_model* m, const double2* y, long long B, int wmode, double* om, double* os, double* oa,
                    double* pk, const double* shift, hipStream_t st);
