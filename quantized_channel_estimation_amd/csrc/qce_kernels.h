// Internal launch interface between the C-ABI layer (qce_capi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>

struct QcePrepareArgs {
  int K, N, M, MP, NP, has_mean, identityA;
  int kind;        // 0: 1 bit, 1: multi-bit, 2: n_bits = inf
  int n_bits;      // multi-bit only
  int quant_kind;  // 0 uniform, 1 lloyd, 2 other (zero gain)
  int beta_first;  // multi-bit Cr: beta = gain[0] (blmmse.py) instead of clip(mean gain, 0, 1)
  double sigma2, delta;
  const double* thr;  // device, 2^b - 1 entries
  const double* lab;  // device, 2^b entries
  const double2* A;   // M x N
  const double2* covs;
  const double2* means;
  const double* logw;
  double2 *Cy, *Cr, *Lw, *Linv, *Aeff, *work, *V, *W, *means_y, *q0, *bvec;
  double *gain, *cconst;
  int* status;
  float* pack32;
  long long stride32;
  double* pack64;
  long long stride64;
};

long long qce_pack_f32_stride(int MP, int NP, int has_mean);
long long qce_pack_f64_stride(int MP, int has_mean);
hipError_t qce_launch_prepare(const QcePrepareArgs& p, hipStream_t st);
hipError_t qce_launch_pack_selective(const QcePrepareArgs& p, hipStream_t st);

struct QceEstArgs {
  long long B;
  int M, N, K, MP, NP, has_mean;
  const double2* y;  // B x M (row stride M)
  const float* pack32;
  long long stride32;
  const double* pack64;
  long long stride64;
  const double* cconst;
};

// 'all' mode, fused responsibilities + LMMSE combination; h = B x N complex128
hipError_t qce_launch_est_all(const QceEstArgs& a, double2* h, hipStream_t st);
// K-shard partial: m, s (B doubles), acc (B x 2N floats, un-normalised, interleaved re/im)
hipError_t qce_launch_est_partial(const QceEstArgs& a, double* m, double* s, float* acc, hipStream_t st);
// weighted log-probabilities lp[b][k] (FP64), row stride K
hipError_t qce_launch_lp(const QceEstArgs& a, double* lp, hipStream_t st);
// selection: mode 0 = proba only, 1 = top-n, 2 = cumulative-p, 3 = argmax(lp)
hipError_t qce_launch_select(long long B, int K, const double* lp, int mode, int n, double p, double* proba,
                             long long* labels, float* wts, hipStream_t st, double* wts64 = nullptr);
int qce_select_max_k();  // widest K qce_launch_select covers (k_select up to 256, k_select_wide beyond)
// FP64 selective-mode LMMSE h = sum_k w64[b][k] (W_k y + b_k), w64 sparse; WT (K x M x N) = transposed filters
// (built from W when transpose, else reused)
hipError_t qce_launch_sparse_f64(long long B, int N, int M, int K, const double2* y, const double* w, const double2* W,
                                 const double2* bvec, double2* WT, bool transpose, double2* h, hipStream_t st);
// h = sum_k wts[b][k] (W_k y_b + b_k)
hipError_t qce_launch_est_weighted(const QceEstArgs& a, const float* wts, double2* h, hipStream_t st);
bool qce_shape_supported(int MP, int NP);         // FP32 fused kernel (M, N <= 64)
bool qce_select_shape_supported(int MP, int NP);  // lp + weighted kernels of the selective modes

// FP16 two-term split kernel (qce_estimate_h2.hip), stream-K scheduled
struct QceH2Args {
  long long B;
  int M, N, K, MP, NP, has_mean;
  int nwg;      // persistent workgroups P
  int R;        // data-parallel rounds of whole tiles
  long long L;  // stream-K tail: work items (tile, component) per workgroup
  double y_scale;
  int* yflag;  // two device ints (k_y_exact): [0] set when some observation is not exact in fp16, [1] the largest
               // biased FP64 exponent of |y * y_scale| (the inexact path's observation scale)
  const double2* y;
  const char* pack;
  long long cstride;  // bytes per component
  const float* sinv;  // K x (NSL + NSW) inverse slice scales (y-scale folded in)
  const double* cconst;
  double2* h;                  // final output (or nullptr with out_partial)
  double *om, *os;             // partial-format output (K-shard path)
  float* oa;
  double *pm, *ps;             // scratch for cut tiles: nwg * 2 * 256 records
  float* pa;
};
long long qce_pack_h2_stride_bytes(int MP, int NP, int has_mean);
hipError_t qce_launch_pack_h2(int K, int M, int N, int MP, int NP, int has_mean, long long cstride, double y_scale,
                              const double2* Linv, const double2* W, const double2* q0, const double2* bvec, char* pack,
                              float* sinv, hipStream_t st);
hipError_t qce_launch_est_h2(const QceH2Args& a, bool out_partial, hipStream_t st);
int qce_h2_blocks_per_cu(int MP, int NP, int has_mean);

// Int8-slice 'all' kernel for quantised observations (qce_estimate_i8.hip): padded M, N <= 64, one workgroup per
// tile of qce_i8_tile(MP, NP) samples over all K components
struct QceI8Args {
  long long B;
  int M, N, K, MP, NP, has_mean;
  int S;      // digit planes per table (3..8)
  int group;  // planes combined in int32 before the FP64 recombination (2; 3 at 1 bit)
  double y_scale;
  const double2* y;
  const signed char* planes;  // K x pstride bytes, fragment-major (see the kernel file)
  long long pstride;
  const double* rowtab;  // K x [scale_L (2MP) | q0 (2MP) | scale_W (2NP) | b (2NP)]
  const double* cconst;
  double2* h;
  // debug launch (dbgL != nullptr): the FP64 raw sums of component dbg_k, (B, 2MP) and (B, 2NP), instead of h
  int dbg_k = 0;
  double *dbgL = nullptr, *dbgW = nullptr;
};
bool qce_i8_shape(int MP, int NP);
int qce_i8_tile(int MP, int NP);  // samples per workgroup
long long qce_pack_i8_bytes(int MP, int NP, int S);  // per component
// k_pack_i8: digit planes, row tables and row exponents (K x (2MP + 2NP) ints) from the resident FP64 tables
hipError_t qce_launch_pack_i8(int K, int M, int N, int MP, int NP, int S, double y_scale, const double2* Linv,
                              const double2* W, const double2* q0, const double2* bvec, signed char* planes,
                              double* rowtab, int* exps, hipStream_t st);
hipError_t qce_launch_est_i8(const QceI8Args& a, hipStream_t st);

// FP64 fused 'all' kernel (qce_estimate_f64.hip): the reference-precision path, stream-K scheduled
struct QceF64Args {
  long long B;
  int M, N, K, MP, NP, has_mean;
  int nwg;      // persistent workgroups P
  int R;        // data-parallel rounds of whole tiles
  long long L;  // stream-K tail: (tile, component) items per workgroup
  const double2* y;
  const char* pack;  // K x qce_pack_f64all_bytes
  const double* cconst;
  double2* h;           // final output (or nullptr with out_partial)
  double *om, *os, *oa;  // partial-format output (K-shard path), oa B x 2N
  double *pm, *ps, *pa;  // scratch for cut tiles: nwg * 2 * tile records
  double* pk = nullptr;   // shifted packed partial B x (2N+2): [s e^{m-shift}, 0, acc e^{m-shift}] (instead of om/os/oa)
  const double* shift = nullptr;  // device pointer: the shared shift M* of the packed partial
  double* pscr = nullptr;  // two-pass 3M kernel (qce_f64g_scratch_doubles > 0): its softmax-weight scratch
  unsigned long long* stamps = nullptr;  // diagnostic builds (-DQCE_STAMPS): per-wave segment cycles
  int waves = 8;  // workgroup shape where M, N <= 64: 8 waves x 1 column tile (two per SIMD), or 4 x 2 (QCE_F64_WAVES=4)
  int g3 = 0;     // 3M tables / kernel: 1 k_est_all_f64g (padded M, N <= 64; 8 waves x 16 samples), 2 k_est_all_f64h
                 // (padded M = N = 128: row halves, y in LDS; 8 waves x 64 samples)
};
// k_est_all_f64h (qce_f64h.hip): the 3M kernel for padded M = N = 128
bool qce_f64h_shape(int MP, int NP);
long long qce_pack_f64h_bytes(int has_mean);
hipError_t qce_launch_pack_f64h(int K, int M, int N, int has_mean, const double2* Linv, const double2* W,
                                const double2* q0, const double2* bvec, double* pack, hipStream_t st);
hipError_t qce_f64h_launch(const QceF64Args& a, bool out_partial, hipStream_t st);
bool qce_f64g_shape(int MP, int NP);
int qce_f64g_waves();  // waves per workgroup of k_est_all_f64g (tile = 16 x waves samples; 8 / waves workgroups per CU)
long long qce_pack_f64g_bytes(int MP, int NP, int has_mean);
// doubles of scratch the 3M kernel needs for a launch of nwg workgroups (K x 128 per workgroup in its two-pass
// form, 0 in the single-pass form)
long long qce_f64g_scratch_doubles(int MP, int NP, int K, long long nwg);
hipError_t qce_launch_pack_f64g(int K, int M, int N, int MP, int NP, int has_mean, const double2* Linv,
                                const double2* W, const double2* q0, const double2* bvec, double* pack,
                                hipStream_t st);
bool qce_f64_shape(int MP, int NP);
int qce_f64_tile(int MP, int NP);  // samples per workgroup tile
long long qce_pack_f64all_bytes(int MP, int NP, int has_mean);
hipError_t qce_launch_pack_f64all(int K, int M, int N, int MP, int NP, int has_mean, const double2* Linv,
                                  const double2* W, const double2* q0, const double2* bvec, double* pack,
                                  hipStream_t st);
hipError_t qce_launch_est_f64(const QceF64Args& a, bool out_partial, hipStream_t st);
hipError_t qce_launch_pack_shifted(long long B, int N, const double* m, const double* s, const double* acc,
                                   const float* acc32, const double* shift, double* pk, hipStream_t st);
// out[0] = max_k cconst[k] (device), the local part of the K-shard shift M*
hipError_t qce_launch_cconst_max(int K, const double* cconst, const int* status, double* out, hipStream_t st);
hipError_t qce_launch_f64_to_f32(const double* a, float* b, long long n, hipStream_t st);
// FP64 'all' mode beyond the fused kernel's 128 (qce_wsum_f64.hip): lp (k_lp_f64) -> weights -> weighted filter sum
struct QceWsumArgs {
  long long B;
  int M, N, K, MP, NP, has_mean;
  const double2* y;
  const char* pack;   // K x qce_pack_wsum_bytes
  const double* wT;   // K x B weights
  double2* out;       // out[b * ostride + ooff + i]
  long long ostride;  // double2 elements per output row
  int ooff;
};
bool qce_wsum_shape(int MP, int NP);
long long qce_pack_wsum_bytes(int MP, int NP, int has_mean);  // per component
hipError_t qce_launch_pack_wsum(int K, int M, int N, int MP, int NP, int has_mean, const double2* W,
                                const double2* bvec, double* pack, hipStream_t st);
// mode 0: proba (K x B), 1: e^{lp - m} with (m, s) -> om / os, 2: e^{lp - shift} with s -> pk[b * pk_stride]
hipError_t qce_launch_wsum_weights(long long B, int K, const double* lp, int mode, const double* shift, double* wT,
                                   double* om, double* os, double* pk, long long pk_stride, hipStream_t st);
hipError_t qce_launch_wsum(const QceWsumArgs& a, hipStream_t st);

hipError_t qce_launch_f32_to_f64(const float* a, double* b, long long n, hipStream_t st);

// flag[0] |= (some y * y_scale is not exactly representable in fp16), flag[1] = largest biased FP64 exponent of
// |y * y_scale| (atomicMax; the caller zeroes both); n = doubles in y
hipError_t qce_launch_y_exact(long long n, const double* y, double y_scale, int* flag, hipStream_t st);

// chunk-streamed FP16 split kernel for padded M or N of 128 / 256 (qce_estimate_h2x.hip)
struct QceH2XArgs {
  long long B;
  int M, N, K, MP, NP, has_mean;
  double y_scale;
  int* yflag;
  const double2* y;
  const char* pack;
  long long cstride;
  const float* sinv;
  const double* cconst;
  double2* h;                  // final output
  double *om, *os;             // K-shard partial output
  float* oa;
  double *rm, *rs;             // split records: ksplit x B (m, s), ksplit x B x 2N acc
  float* ra;
};
bool qce_h2x_shape(int MP, int NP);
long long qce_h2x_pad_bytes();  // extra bytes the pack allocation needs (chunk overrun)
int qce_h2x_tile();
int qce_h2x_row_chunks(int MP, int NP);
hipError_t qce_launch_est_h2x(const QceH2XArgs& a, int ksplit, bool out_partial, hipStream_t st);

// Fourier-domain path for (block-)circulant mixtures with A = I (qce_fft.hip)
struct QceFftPrepArgs {
  int N, n1, n2, K;
  double s2;
  int kind, n_bits, quant_kind;
  double delta;
  const double *thr, *lab, *logw, *ceig;
  const double2 *col0, *mspec;
  double* rinvT;   // N x K
  double2* uT;     // N x K
  double* cprime;  // K
  double* wT;      // K x N
  double2* bT;     // K x N
  double* gain;    // K
  int* status;     // K
};
struct QceFftEstArgs {
  long long B;
  int N, n1, n2, K, has_mean;
  const double2* y;
  const double* rinvT;
  const double2* uT;
  const double* cprime;
  const double* wT;
  const double2* bT;
  const double* wts;  // FP64 selection weights (out = 2; k_select's wts64)
  double2* h;
  double* lp;        // out = 1
  double *om, *os;   // out = 3, 4
  float* oa;         // out = 3: f32 (B, 2N); out = 4: the same buffer holds an f64 (B, 2N) accumulator
  // MFMA kernel tables (qce_fft_mfma.hip, storage order, components padded to Kp)
  int Kp;
  const double *pr, *pur, *pui, *pc, *pw, *pbr, *pbi;
  int cu;  // compute units of the device (persistent grid of k_fft_wave / k_fft_wreg)
};
bool qce_fft_pow2(int v);
int qce_fft_tile(int N, int K);  // 0: no tile fits (K too large)
hipError_t qce_launch_fft_struct(int K, int N, int n1, int n2, double tol, const double2* covs, const double2* means,
                                 double* ceig, double2* col0, double2* mspec, int* bad, hipStream_t st);
hipError_t qce_launch_fft_prep(const QceFftPrepArgs& a, hipStream_t st);
// out: 0 'all' h, 1 lp, 2 weighted h, 3 K-shard partial (f32 acc), 4 K-shard partial (f64 acc)
hipError_t qce_launch_fft_est(const QceFftEstArgs& a, int out, hipStream_t st);
// MFMA Fourier kernel (qce_fft_mfma.hip): N in {16, ..., 256}; out 0 'all' h, 3 / 4 K-shard partial (f32 / f64)
bool qce_fft_mfma_shape(int N);
int qce_fft_kpad(int K);
hipError_t qce_launch_fft_pack(const QceFftEstArgs& a, const double* rinvT, const double2* uT, const double* cprime,
                               const double* wT, const double2* bT, hipStream_t st);
hipError_t qce_launch_fft_mfma(const QceFftEstArgs& a, int out, hipStream_t st);

// Fourier-domain path with pilots, A = kron(x, I_N), 2 <= P <= 4 (qce_fft_pilot.hip); components padded to Kp
struct QceFftpPrepArgs {
  int N, n1, n2, K, Kp, P, has_mean;
  double2 x[4];  // the pilot vector
  double s2;
  int kind, n_bits, quant_kind;
  double delta;
  const double *thr, *lab, *logw, *ceig;
  const double2 *col0, *mspec;
  double* tabL;    // lp operand [Kp / 16][TL][N][16], TL = P^2 (+ 2 P with means)
  double* cprime;  // Kp (padding: -inf)
  double* tabW;    // filter operand [N / 16][TF][Kp][16], TF = 2 P (+ 2 with means)
  int* status;     // K
};
struct QceFftpEstArgs {
  long long B;
  int N, n1, n2, K, Kp, P, has_mean;
  const double2* y;  // B x P N
  const double *tabL, *cprime, *tabW;
  const double* wts;  // FP64 selection weights (out = 2)
  double2* h;
  double* lp;  // out = 1
};
bool qce_fftp_shape(int N, int P, int K);  // the kernels cover (N, P) and the LDS tile fits at K components
int qce_fftp_kpad(int K);
long long qce_fftp_tabl_doubles(int N, int P, int Kp, int has_mean);
long long qce_fftp_tabw_doubles(int N, int P, int Kp, int has_mean);
hipError_t qce_launch_fftp_prep(const QceFftpPrepArgs& a, hipStream_t st);
// out: 0 'all' h, 1 lp, 2 weighted h
hipError_t qce_launch_fftp_est(const QceFftpEstArgs& a, int out, hipStream_t st);

// Observation generation / quantisation (qce_observe.hip; utils.py:189-203, :241-251)
struct QceObserveArgs {
  long long B;
  int M, N;
  const double2* A;  // M x N, nullptr = identity (M == N)
  const double2* h;  // B x N
  const double2* w;  // B x M supplied noise (noise == 1)
  int noise;         // 0 none, 1 supplied, 2 generated (Philox, seed, element offset)
  double noise_scale;
  unsigned long long seed, offset;
  int kind;  // 0: 1 bit, 1: multi-bit (thr / lab), 2: unquantised
  const double* thr;
  const double* lab;
  int nthr;
  double2* y;  // B x M
};
hipError_t qce_launch_observe(const QceObserveArgs& a, hipStream_t st);

// Random-SNR observations and encoder features (qce_observe_rows.hip; utils.py:254-318, vae.py:46-53, :89-94)
#define QCE_ROWS_MAX_SNRS 64
#define QCE_ROWS_TABLE_LDS (32 * 1024)  // per-SNR quantiser tables are held in LDS up to this many bytes
struct QceObserveRowsArgs {
  long long B;
  int M, N;
  const double2* A;    // M x N dense, nullptr = identity (M == N) or kron(x, I_N) (P > 0)
  int P;               // > 0: A = kron(x, I_N), M = P N, x in xk; 0 otherwise
  const double2* xk;   // device, P entries
  const double2* h;    // B x N
  const double2* w;    // B x M supplied noise (noise == 1)
  int noise;           // 0 none, 1 supplied, 2 generated (element counter (row_offset + b) M + m)
  unsigned long long seed, row_offset;
  int S;               // number of SNRs, <= QCE_ROWS_MAX_SNRS
  const double* scales;  // device, S noise scales 10^(-snr / 20)
  const double* cdf;     // device, S cumulative probabilities, or nullptr (uniform draw)
  const int* idx_in;     // B supplied SNR indices, or nullptr (drawn: row counter row_offset + b)
  int* idx_out;          // B
  int kind;              // 0: 1 bit, 1: multi-bit, 2: unquantised
  int nthr;              // L - 1 (multi-bit)
  const double* thr;     // device, S x (L - 1)
  const double* lab;     // device, S x L
  int out;               // 0: y complex128 (B, M); 1: raw features, 2: DFT features, float (B, M / N, 2 N)
  double2* y;
  float* feat;
};
bool qce_observe_rows_feature_shape(int N);  // N in {16, 32, 64, 128, 256}
hipError_t qce_launch_observe_rows(const QceObserveRowsArgs& a, hipStream_t st);
int qce_sq_err_scratch();
hipError_t qce_launch_sq_err(long long n, const double2* a, const double2* b, double* part, double* out,
                             hipStream_t st);

// EM training (qce_em.hip; gmm_cplx_bussgang.py:612-790)
struct QceEmPlan {
  int C = 0;      // stats chunks of 1024 samples
  int NT = 0;     // 16-wide feature tiles
  int nblk = 0;   // 64 x 64 output blocks
  int chunk = 0;  // samples per covariance workgroup
  int C2 = 0;     // covariance chunks
  size_t stat_doubles = 0, part_elems = 0;
};
QceEmPlan qce_em_plan(long long B, int N, int K, int diag);
struct QceEmArgs {
  long long B;
  int N, K, diag, zero_mean;
  double reg;
  QceEmPlan plan;
  const double2* X;  // B x N
  const double* R;   // B x K responsibilities
  double* stats;     // plan.stat_doubles
  double2* part;     // plan.part_elems
  double* nk;        // K
  double2* means;    // K x N
  double2* covs;     // K x N x N ('full')
  double* diag_out;  // K x N ('diag')
};
hipError_t qce_launch_em_mstep(const QceEmArgs& a, hipStream_t st);
int qce_mean_scratch();
hipError_t qce_launch_em_resp(long long B, int K, const double* lp, double* resp, double* lse, double* part,
                              double* mean_out, hipStream_t st);

// h_b = W_c y_b + b_c with c = comp[b] (comp == nullptr: c = b) — per-sample ("genie") filters
hipError_t qce_launch_est_assigned(long long B, int N, int M, int K, const double2* y, const long long* comp,
                                   const double2* W, const double2* bvec, double2* h, hipStream_t st);

// batched row-major complex GEMM C = alpha op(A) op(B) + beta C (op 0 = N, 1 = T, 2 = C^H); supported
// (opa, opb): (0,0) (0,2) (2,0) (0,1).  Strides sA/sB/sC per batch entry (0 = shared operand).
hipError_t qce_zgemm_batched(int opa, int opb, int m, int n, int k, double2 alpha, const double2* A, int lda,
                             long long sA, const double2* B, int ldb, long long sB, double2 beta, double2* C, int ldc,
                             long long sC, int batch, hipStream_t st);
// Toeplitz inverse-EM covariance step (qce_em.hip; gmm_cplx_bussgang.py:792-826)
//   theta_kp = Re diag(F2 Mx_k F2^H)_p; init: sigma = max(theta, reg); else sigma += sigma^2 theta, max reg
hipError_t qce_launch_inv_em_sigma(int K, int N, int P, const double2* G, const double2* F2, double* sigma, double reg,
                                   int init, hipStream_t st);
//   C_k = F2^H diag(sigma_k) F2 + reg I
hipError_t qce_launch_inv_em_cov(int K, int N, int P, const double2* F2, const double* sigma, double reg, double2* C,
                                 hipStream_t st);

// SCM channels (qce_scm.hip; scm_helper.py:17-84, SCMMulti.py:30-56)
int qce_scm_max_path();
hipError_t qce_launch_scm(long long B, int n_coh, int N, int n_path, double sigma, const double* gains,
                          const double* angles, const double2* x, unsigned long long seed, float2* h, float2* t,
                          hipStream_t st);

// statistical rate lower bound (qce_rate.hip; Bussgang_GMM.py:146-162)
int qce_rate_scratch();
hipError_t qce_launch_rate(long long B, int N, const double2* he, const double2* h, const double* buss,
                           const double2* Cq, double clip, double2* inner, double* den2, double* part, double* stat,
                           hipStream_t st);
// VAE-parameterised Bussgang LMMSE in the Fourier domain (qce_vae.hip; estimators/vae.py:368-431)
#define QCE_VAE_MAX_PILOTS 4
#define QCE_VAE_LDS_BUDGET (72 * 1024)  // LDS per workgroup: two workgroups per CU
struct QceVaeArgs {
  long long B;
  int N, P;           // N a power of two in [16, 256], P <= QCE_VAE_MAX_PILOTS
  int kind, n_bits;   // 0: 1 bit, 1: uniform n_bits, 2: no quantisation
  double s2, delta;   // noise variance, uniform quantiser step
  double k1, k2, k3;  // the reference's float32 constants sqrt(2/pi), delta/sqrt(pi), 2/pi
  double2 x[QCE_VAE_MAX_PILOTS];  // pilot vector: A = kron(x, I_N)
  const void* lv;     // B x N log-variances, float (lv_f32) or double
  int lv_f32;
  const double2* y;   // B x (P N), pilot-major
  double2* h;         // B x N
  int* status;        // |= 1 when some bin's P x P matrix is not positive definite
  int TS;             // samples per workgroup (set by the launcher)
};
hipError_t qce_launch_vae(const QceVaeArgs& a, hipStream_t st);
// The VAE's inference network in one kernel (qce_vae_net.hip; estimators/vae.py:161-172 and :294-309 forward_nosamp):
// features, pilot convolutions, encoder (mu only) and decoder for a tile of 16 rows per workgroup.
#define QCE_VAE_NET_MAX_LAYERS 8   // per MLP
#define QCE_VAE_NET_MAX_CONVS 4
#define QCE_VAE_NET_MAX_WIDTH 512
#define QCE_VAE_NET_ROWS 16        // rows per workgroup: the M of v_mfma_f32_16x16x4_f32
struct QceVaeNetLayer {
  int ksteps;   // ceil(in / 4): MFMA k-steps (the packed weights are zero beyond in)
  int ntiles;   // ceil(out / 16): output column tiles (zero weights and bias beyond out)
  int w_off;    // floats into `packed`: ntiles x ksteps x 64, lane-major per (tile, k-step)
  int b_off;    // floats into `packed`: 16 ntiles
  int relu;
};
struct QceVaeNetArgs {
  long long B;
  int N, P;               // P: rows of N complex values per sample in `in` (1 for a genie network)
  int L;
  int dft;                // 1: unitary DFT features, 0: [Re | Im] of the input itself
  int nconv;              // pilot convolutions (kernel size 1), channels conv_ch[0] = P .. conv_ch[nconv] = 1
  int conv_ch[QCE_VAE_NET_MAX_CONVS + 1];
  int conv_off[QCE_VAE_NET_MAX_CONVS];  // floats into `raw`: weight (out, in) row-major, then bias (out)
  int nenc, nlayers;      // layers [0, nenc) are the encoder's (the last keeps its first L outputs), the rest the decoder's
  QceVaeNetLayer layer[2 * QCE_VAE_NET_MAX_LAYERS];
  int stride;             // floats per row of an activation buffer: >= every padded width, = 4 mod 64
  int spp;                // samples transformed per pass (spp P (N + 1) complex values of staging)
  const float* raw;       // the caller's flat weights (the convolutions are read from here)
  const float* packed;
  const double2* in;      // B x (P N)
  float* mu;              // B x L, or nullptr
  float* lv;              // B x N
};
size_t qce_vae_net_lds(const QceVaeNetArgs& a);
hipError_t qce_launch_vae_net(const QceVaeNetArgs& a, hipStream_t st);
// VAE training: reparameterisation and the fused row ELBO with its gradient (qce_vae_train.hip; estimators/vae.py:280-281,
// :312-365)
#define QCE_VAE_MAX_LATENT 128
struct QceVaeElboArgs {
  long long B, T;      // rows of the batch; rows of t and entries of snr (the range of index)
  int N, L;            // N a power of two in [16, 256], 1 <= L <= QCE_VAE_MAX_LATENT
  int mode;            // 0: genie / noisy, 1: real
  int n_bits;          // mode 1: 1..8 (uniform quantiser), 0 = no quantisation
  double step;         // mode 1: the standard uniform step of n_bits
  float sqrt_pi_f;     // sqrt(float(pi)) as float32: k2 = float(delta) / sqrt_pi_f
  const float* enc;    // B x 2L = [mu | s]
  const float* dec;    // B x N
  const float* t;      // T x 2N = [tr | ti]
  const int* index;    // B, or nullptr (row b uses target row b)
  const double* snr;   // T (mode 1), dB
  double* rows;        // B row ELBOs
  float* g_enc;        // B x 2L
  float* g_dec;        // B x N
};
bool qce_vae_train_shape(int N, int L);
hipError_t qce_launch_vae_sample(const float* enc, const float* eps_in, long long B, int L, unsigned long long seed,
                                 unsigned long long row_offset, float* z, float* eps_out, hipStream_t st);
hipError_t qce_launch_vae_sample_bwd(const float* enc, const float* eps, const float* gz, long long B, int L,
                                     float* g_enc, hipStream_t st);
hipError_t qce_launch_vae_elbo(const QceVaeElboArgs& a, hipStream_t st);
// The fused VAE training step (qce_vae_step.hip): k_vae_step (gather, forward, row ELBO, backward, per-tile partial
// gradients) and k_vae_update (tile-ordered reduction, skip rule, Adam).  Parameters are one flat float32 array in
// state-dict order: per pilot convolution weight (out, in) then bias, then per encoder and decoder layer weight
// (out, in) row-major then bias.
#define QCE_VAE_STEP_LDS_LIMIT (160 * 1024)  // LDS bytes of one workgroup (one CU of gfx950)
#define QCE_VAE_STEP_MAX_CONV_PARAMS (QCE_VAE_NET_MAX_CONVS * (QCE_VAE_MAX_PILOTS * QCE_VAE_MAX_PILOTS + QCE_VAE_MAX_PILOTS))
#define QCE_VAE_LOSS_SKIP 1000.0             // a step whose loss is NaN or above this updates nothing (vae.py:120-121)
struct QceVaeStepLayer {
  int in, out;        // W is (out, in)
  int w_off, b_off;   // floats into the flat parameters (and into a row of partials)
  int relu;           // ReLU on the output
  int src, dst;       // LDS float offsets of the input and the output activations (16 rows each)
  int s_src, s_dst;   // their row strides: the width rounded up to 16, plus 4
};
struct QceVaeStepArgs {
  long long B, n_x, T;     // batch rows; rows of x; rows of t (and entries of snr)
  int N, P, L;             // P: channels of a row of x (1 without convolutions)
  int mode;                // loss: 0 genie / noisy, 1 real
  int n_bits;              // mode 1: 1..8, 0 = no quantiser
  double step;             // mode 1: the standard uniform step
  float sqrt_pi_f;
  int nconv;
  int conv_ch[QCE_VAE_NET_MAX_CONVS + 1];
  int conv_off[QCE_VAE_NET_MAX_CONVS];  // floats into the parameters: weight (out, in), then bias (out)
  int n_conv_params;
  int nenc, nlayers;       // layers [0, nenc): encoder (the last gives [mu | s]), the rest: decoder
  QceVaeStepLayer layer[2 * QCE_VAE_NET_MAX_LAYERS];
  // LDS float offsets: raw x tile (16 x P x 2N, with convolutions), z's eps (16 x L), the KL gradient (16 x 2L), the two
  // delta buffers (16 x s_delta each); the convolutions' reduction staging shares the bytes of the delta buffers' tail
  int x_off, eps_off, kl_off, d0_off, d1_off, s_delta, red_off;
  unsigned lds_bytes;
  int n_params;
  const float* w;          // flat parameters
  const float* x;          // (n_x, P, 2N) features
  const float* t;          // (T, 2N) targets
  const int* index;        // (B,) rows of x / t, clamped; or NULL: row b
  const double* snr;       // (T,), mode 1
  const float* eps;        // (B, L), or NULL: drawn from (seed, row_offset)
  unsigned long long seed, row_offset;
  double* rows;            // (B,) row ELBOs
  float* partials;         // (tiles, n_params)
  const long long* count;  // Adam's step count; the kernel copies it to *count_snap for k_vae_update
  long long* count_snap;
};
struct QceVaeUpdateArgs {
  long long B;
  int tiles, n_params;
  const float* partials;
  const double* rows;
  float *w, *m, *v;             // NULL w: no update (gradients only)
  const long long* count_snap;  // the step count before this step
  long long* count;
  double lr;
  double* loss_out;             // losses[slot], or the caller's scalar
  int* skipped_out;             // skipped[slot], or NULL
  float* grads_out;             // (n_params,) reduced gradient, or NULL
};
hipError_t qce_launch_vae_step(const QceVaeStepArgs& a, hipStream_t st);
hipError_t qce_launch_vae_update(const QceVaeUpdateArgs& a, hipStream_t st);
// Bussgang LS with column-orthogonal A_eff (qce_genie.hip; estimators/LS.py)
hipError_t qce_launch_ls(long long B, int N, int M, const double2* y, const long long* comp, const double2* Aeff,
                         double2* h, hipStream_t st);
// Pseudo-inverses P_c = (A_eff^H A_eff)^{-1} A_eff^H of full-column-rank A_eff (qce_genie.hip; LS.py general A)
hipError_t qce_launch_rate_mf(long long B, int N, const double2* he, const double2* h, const double* buss,
                              const double2* Cq, const double2* Cqi, double* rate, double* sum, hipStream_t st);
// Gauss-Jordan inverse per component: direct = 0 -> (A^H A)^-1 A^H (M >= N), 1 -> A^-1 (A Hermitian PD, M == N);
// bad[c] = first failing pivot + 1 (0 = ok)
hipError_t qce_launch_ls_pinv(int K, int N, int M, int direct, const double2* Aeff, double2* T, double2* P,
                              double2* bzero, int* bad, hipStream_t st);
