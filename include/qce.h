/*
 * qce.h — C ABI of the MI355X-native Bussgang-GMM channel estimator (libqce.so).
 *
 * This is the drop-in boundary for the hot path of benediktfesl/Quantized_Channel_Estimation:
 * the per-SNR precompute and the per-batch estimate of `Gmm_nbit` (modules/gmm_cplx_bussgang.py)
 * and its twin `Gmm_quant` (modules/gmm_cplx_quant.py:190-457).  The Python host class
 * `quantized_channel_estimation_amd.Gmm_nbit` binds these entry points through ctypes
 * (INTEGRATION.md shows the binding a maintainer of the reference would add).
 *
 * Conventions
 *  - complex numbers are interleaved (re, im) doubles, numpy complex128 layout; all arrays are
 *    row-major (C order) and contiguous;
 *  - `io` selects where the caller's I/O buffers live: QCE_IO_HOST (host memory, the call is
 *    synchronous) or QCE_IO_DEVICE (device memory of the model's device, e.g. a torch tensor's
 *    data_ptr(); the call is asynchronous on `stream`, NULL = the model's own stream);
 *  - the library owns the per-model device tables; a model is bound to one device and is not
 *    thread-safe (use one model per thread/stream);
 *  - every entry point returns a status code (QCE_OK = 0); `qce_last_error()` returns the message
 *    of the last failure on the calling thread.  No C++ exception crosses the ABI.
 */
#ifndef QCE_H
#define QCE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qce_model qce_model;

/* status codes */
#define QCE_OK 0
#define QCE_EARG 1     /* invalid argument (shape, pointer, mode)            -> ValueError          */
#define QCE_ECHOL 2    /* Cr_k not positive definite (gmm_cplx_bussgang.py:43-46) -> ValueError      */
#define QCE_ENOTIMPL 3 /* configuration the kernels do not cover          -> NotImplementedError */
#define QCE_EHIP 4     /* HIP runtime failure                              -> RuntimeError        */
#define QCE_ESTATE 5   /* call order (estimate before prepare)             -> RuntimeError        */
#define QCE_ECOMM 6    /* communicator / collective failure (RCCL or host transport) -> RuntimeError */

/* estimate modes (gmm_cplx_bussgang.py:197-242) */
#define QCE_MODE_ALL 0  /* 'all': sum of all responsibility-weighted LMMSE estimates   (:220-228) */
#define QCE_MODE_TOPN 1 /* int n: top-n by responsibility, renormalised; n == 1 -> argmax (:197-219) */
#define QCE_MODE_CUMP 2 /* float p: shortest descending prefix with cumulative prob >= p (:229-242) */

/* quantiser kinds for multi-bit n_bits (gmm_cplx_bussgang.py:281-284) */
#define QCE_QUANT_UNIFORM 0
#define QCE_QUANT_LLOYD 1
#define QCE_QUANT_OTHER 2 /* any other string: the reference leaves the Bussgang gain at 0 */

/* model options (qce_model_set_option) */
#define QCE_OPT_BETA_FIRST 1 /* multi-bit Cr = g_0^2 Cy + (1 - g_0^2) diag(Cy) with the first Bussgang gain
                                (estimators/blmmse.py:53, :86) instead of clip(mean gain, 0, 1)
                                (gmm_cplx_bussgang.py:304-307); value != 0 enables */

#define QCE_OPT_PRECISION 2 /* arithmetic of the dense 'all' mode and the K-shard partial: QCE_PRECISION_F64 (default,
                               the reference's complex128 arithmetic: FP64 MFMA products, FP64 accumulation and
                               softmax) or QCE_PRECISION_FAST (fp16 two-term split products with fp32 accumulation,
                               ~1e-7 relative; an opt-in throughput mode) */
#define QCE_PRECISION_F64 0
#define QCE_PRECISION_FAST 1
#define QCE_PRECISION_INT8 2 /* quantised observations (1 bit, uniform 2..7 bits), dense model, padded M, N <= 64: the
                                tables cut into QCE_OPT_INT8_SLICES base-128 digit planes, exact int32 products on the
                                i8 MFMA, FP64 recombination / softmax / combine.  Any other model is prepared as under
                                QCE_PRECISION_F64.  A sample whose scaled observation is not an integer up to 127 gets
                                NaN in its whole output row; the K-shard partial calls return QCE_ENOTIMPL. */
#define QCE_OPT_RESERVE_CUS 3 /* CUs the persistent estimate kernels leave free (value >= 0; default 0): room for the
                                 collective kernels of a concurrent communication stream (qce_kshard_create sets it on
                                 the shard's models for RCCL at world > 1).  Keeps the prepared state. */

#define QCE_OPT_INT8_SLICES 4 /* digit planes per table under QCE_PRECISION_INT8: an integer in 3..8 (default 7, the
                                 smallest count whose error sits on the FP64 rounding floor; each plane less costs a
                                 factor 128 in accuracy).  Drops the prepared state. */

#define QCE_OPT_FOURIER_PILOTS 5 /* value != 0 (default 0): a (block-)circulant model observed through A = kron(x, I_N)
                                    with 2 <= P <= 4 pilots, N a power of two in 16..256 and P N <= 512 is prepared
                                    and estimated in the Fourier domain (per-bin P x P tables, QCE_KERNEL_FOURIER_PILOTS)
                                    instead of the dense families at M = P N.  A must be exactly kron(x, I_N): every
                                    off-diagonal entry of every N x N block zero (no tolerance), one value on each
                                    block's diagonal.  Anything else is prepared as without the option.  The K-shard partial
                                    calls return QCE_ENOTIMPL on such a prepare.  Drops the prepared state. */

#define QCE_IO_HOST 0
#define QCE_IO_DEVICE 1

int qce_version(void);
/* Digest of the sources this library was built from (build.py: sha256 of the csrc .hip / .h files and qce.h). */
const char* qce_build_id(void);
const char* qce_last_error(void);
int qce_device_count(int* count);

/* Model parameters after `Gmm_nbit.fit` (gmm_cplx_bussgang.py:96-163): means_cplx (K,N) c128,
 * covs_cplx (K,N,N) c128, gm.weights_ (K,) f64.  Replaces the attribute bag the reference keeps in
 * its sklearn GaussianMixture (:86-94).  N <= 256 (padded internally to 16/32/64/128/256), K <= 4096 for
 * the selective modes and the proba / labels outputs (any K for 'all').  The structure of the covariances is
 * detected here (qce_model_structure). */
int qce_model_create(int K, int N, const double* means_cplx, const double* covs_cplx, const double* weights,
                     int device, qce_model** out);
int qce_model_destroy(qce_model* model);
/* Replace the parameters of a model in place (same K, N; e.g. between EM iterations): re-uploads
 * means / covariances / weights, re-detects the structure and drops the prepared state. */
int qce_model_set_params(qce_model* model, const double* means_cplx, const double* covs_cplx, const double* weights);

/* Per-SNR precompute: `_prepare_for_prediction` (gmm_cplx_bussgang.py:246-328).
 * A: (M,N) c128 observation matrix, or NULL for the identity (estimate_from_y :191-192).
 * n_bits: 1..16 (uniform; beyond 8 bits the step is the reference's asymptote 4 sqrt(b) 2^-b,
 * uniform_quantizer.py:15-21; lloyd: 1..8) or +INFINITY (np.inf).  thresholds (2^b-1) / labels (2^b) are the
 * quantiser tables of the lloyd kind (lloyd_max_quantizer.py:24-37); NULL otherwise.
 * Runs asynchronously on `stream` (NULL = the model's stream; pass the stream later estimates use so a prepare
 * never overwrites tables an in-flight estimate still reads); no host synchronisation.  The per-component
 * Cholesky status is copied behind the prepare's kernels and read at the next call that synchronises anyway
 * (host-I/O estimates, qce_log_prob, qce_get_tables, qce_synchronize, host-I/O qce_cconst_max), which returns
 * QCE_ECHOL if some Cr_k is not positive definite (:43-46).  Device-I/O estimates issued in between compute on
 * NaN tables; device-I/O callers read the status through qce_cconst_max (it writes +inf on a failure). */
int qce_prepare(qce_model* model, const double* A, int M, double snr_db, double n_bits, int quant_kind,
                const double* thresholds, const double* labels, int n_levels, void* stream);

/* Channel estimates: `estimate_from_y` (gmm_cplx_bussgang.py:166-243) for y (B,M) c128 -> h (B,N) c128.
 * mode/mode_param: QCE_MODE_ALL; QCE_MODE_TOPN with n; QCE_MODE_CUMP with p. */
int qce_estimate(qce_model* model, const double* y, int64_t B, int mode, double mode_param, double* h_out, int io,
                 void* stream);

/* `_estimate_weighted_log_prob` (:369-386) -> lp (B,K) f64; `predict_proba_cplx` (:351-367) -> proba (B,K);
 * `_predict_cplx` (:335-349) -> labels (B,) int64.  Any output pointer may be NULL. */
int qce_log_prob(qce_model* model, const double* X, int64_t B, double* lp_out, double* proba_out,
                 int64_t* labels_out, int io, void* stream);

/* K-shard partial of the 'all' mode for the components this model holds: per sample the running max
 * m (B,) f64, the sum s = sum_k exp(lp_k - m) (B,) f64 and acc = sum_k exp(lp_k - m) (W_k y + b_k)
 * (B, 2N) f32 interleaved; h = (sum_g acc_g e^{m_g}) / (sum_g s_g e^{m_g}). */
int qce_estimate_partial(qce_model* model, const double* y, int64_t B, double* m_out, double* s_out, float* acc_out,
                         int io, void* stream);

/* The same partial with an FP64 accumulator acc (B, 2N) f64 interleaved — the format the K-shard combine
 * all-reduces (one SUM of (s, acc) under a shared shift, sharding.py). */
int qce_estimate_partial_f64(qce_model* model, const double* y, int64_t B, double* m_out, double* s_out, double* acc_out,
                             int io, void* stream);

/* The K-shard partial scaled to a shift shared by all shards and packed for one SUM collective:
 * packed_out (B, 2N+2) f64, row b = [s_b e^{m_b - shift}, 0, acc_b e^{m_b - shift} (2N interleaved)].
 * shift: one double where `io` says (device memory for QCE_IO_DEVICE, so the shift can come from a device-side
 * collective without a host round trip).  With shift = max over ALL components of cconst (>= every lp, the quad
 * form is >= 0) the element-wise sum over shards of these rows gives h_b = acc / s exactly (rows whose sum
 * underflows to s = 0 need the two-step combine of the unshifted partials). */
int qce_estimate_partial_shifted(qce_model* model, const double* y, int64_t B, const double* shift, double* packed_out,
                                 int io, void* stream);

/* out[0] = max_k cconst_k of the last prepare (this shard's part of the shift above; the caller reduces it over
 * shards with a MAX collective), or +INFINITY if the prepare's Cholesky factorisation failed for some component:
 * the failure then travels with the shift through the MAX collective to every shard (sharding.py raises the
 * reference's ValueError).  `out` where `io` says; device I/O is asynchronous on `stream`, host I/O synchronises
 * and returns QCE_ECHOL on a failure. */
int qce_cconst_max(qce_model* model, double* out, int io, void* stream);

/* Per-SNR tables for state mirroring (the reference mutates gm.means_, gm.covariances_,
 * gm.precisions_cholesky_, :262-313) and tests.  Host pointers, any may be NULL:
 * means_y (K,M), Cy (K,M,M), Cr (K,M,M), P (K,M,M) = (L^-1)^H, A_eff (K,M,N), W (K,N,M),
 * b (K,N), cconst (K,) = -M log(pi) + 2 log det P_k + log w_k. */
int qce_get_tables(qce_model* model, double* means_y, double* Cy, double* Cr, double* P, double* A_eff, double* W,
                   double* b, double* cconst);

/* Dimensions of the prepared state (M <= 256): M (0 before the first prepare). */
int qce_model_info(qce_model* model, int* K, int* N, int* M, int* device);

/* Structure of the mixture found at creation: every C_k is block-circulant for kron(F_n1, F_n2) (n1 = 1:
 * circulant, the fits of gmm_cplx_bussgang.py:104-133), or n1 = n2 = 0.  With A = I such a model is
 * prepared and estimated in the Fourier domain (per-bin tables; fourier_active = 1 after such a prepare).
 * With QCE_OPT_FOURIER_PILOTS set the same holds for A = kron(x, I_N), 2 <= P <= 4 pilots (per-bin P x P tables;
 * fourier_active = 1, qce_model_kernel reports QCE_KERNEL_FOURIER_PILOTS).
 * Environment QCE_FFT=0 keeps every prepare on the dense path. */
int qce_model_structure(qce_model* model, int* n1, int* n2, int* fourier_active);
/* The 'all'-mode kernel family the last prepare selected (diagnostics, benchmarks): */
#define QCE_KERNEL_NONE 0     /* not prepared */
#define QCE_KERNEL_F64_4M 1   /* k_est_all_f64: real 2x2 embedding, FP64 MFMA (padded M, N up to 128) */
#define QCE_KERNEL_F64_3M 2   /* k_est_all_f64g: Gauss 3-product complex multiply, FP64 MFMA (padded M, N <= 64) */
#define QCE_KERNEL_F64_WIDE 3 /* k_lp_f64 + k_wsum_f64 (padded 256) */
#define QCE_KERNEL_BIG 4      /* GEMM path, N or M in (256, 4096] */
#define QCE_KERNEL_FOURIER 5  /* (block-)circulant models in the Fourier basis */
#define QCE_KERNEL_FAST 6     /* precision 'fast': fp16 two-term split */
#define QCE_KERNEL_INT8 7     /* precision 'int8': k_est_all_i8, int8 digit planes on the i8 MFMA */
#define QCE_KERNEL_FOURIER_PILOTS 8 /* (block-)circulant models with A = kron(x, I_N) in the Fourier basis */
int qce_model_kernel(qce_model* model, int* kind);

/* Diagnostics of a model prepared onto QCE_KERNEL_INT8 (QCE_ESTATE otherwise): for component k and y (B,M) c128, the
 * FP64 sums raw = sum_s 128^s (D_s ti) of the two digit-plane products before the power-of-two row scale and before
 * 1 / y_scale -- raw_L (B, 2 MP) and raw_W (B, 2 NP), MP / NP the padded M / N (16, 32 or 64) -- and the row exponents
 * exps (2 MP + 2 NP ints: E(Linv_k) rows, then E(W_k) rows).  Host pointers, any output may be NULL; synchronises. */
int qce_debug_i8_products(qce_model* model, const double* y, int64_t B, int k, double* raw_L, double* raw_W,
                          int* exps);

/* Observations on the device (model-free): `get_observation_nbit` (utils.py:241-251) with `quant`
 * (utils.py:189-203):  y = Q(A h + noise_scale * w).
 * h (B,N) c128; A (M,N) c128 host array or NULL for the identity (then M == N); y_out (B,M) c128.
 * noise_kind: 0 none (pure quantiser, `quant`), 1 w supplied in `noise` (B,M) c128 — the reference's
 * crandn draw, result bit-identical to numpy for A = NULL —, 2 generated on the device: circular
 * CN(0,1) from Philox4x32-10 keyed by `seed`, complex element e of the batch uses counter offset + e.
 * n_bits: 1 (sign law), +INFINITY (no quantisation), else labels[np.digitize(.)] with thresholds
 * (n_levels - 1, increasing) and labels (n_levels) host arrays.  h / noise / y_out live where `io` says;
 * `stream` NULL = the null stream of `device`. */
int qce_observe(const double* h, int64_t B, int N, const double* A, int M, double noise_scale, int noise_kind,
                const double* noise, uint64_t seed, uint64_t offset, double n_bits, const double* thresholds,
                const double* labels, int n_levels, double* y_out, int device, int io, void* stream);

/* Random-SNR observations and the VAE encoder's input features (model-free): `get_observation_nbit_randSNR`
 * and its torch variants (utils.py:254-318) with the feature step of estimators/vae.py:46-53 / :89-94, one launch:
 *   i_b = snr_index_in[b], or drawn from {0..S-1}: cdf (S, host, cumulative probabilities) or NULL for uniform;
 *   y_b = Q_{i_b}(A h_b + noise_scales[i_b] * w_b);  snr_index_out[b] = i_b (int32, always written).
 * h, A, M, noise_kind, noise and n_bits as for qce_observe; noise_scales (S,) host, S <= 64.  Multi-bit: thresholds
 * (S, n_levels - 1) and labels (S, n_levels) host arrays, one table per SNR, 2 <= n_levels <= 256.
 * Generated draws (Philox4x32-10 keyed by seed): the noise of complex element (b, m) uses counter
 * (row_offset + b) M + m of qce_observe's noise stream (S = 1 equals qce_observe with offset = row_offset M), the
 * index of row b uses counter row_offset + b of a separate stream: u in [0, 1), i_b = #{cdf[i] <= u} clamped to
 * S - 1 (uniform: floor(u S)).  Generating rows [B1, B) with row_offset = B1 reproduces the one-shot rows.
 * out_kind: QCE_OUT_Y, out = y (B, M) c128; QCE_OUT_FEATURES_RAW / _DFT, out = float32 (B, M / N, 2 N), row (b, p) =
 * [Re f | Im f] with f = y_b[pN:(p+1)N], or its unitary DFT (FP64 transform, rounded to float at the store); features
 * need N in {16, 32, 64, 128, 256} and N | M, else QCE_ENOTIMPL, and a 16-byte aligned `out`.
 * h / noise / snr_index_in / snr_index_out / out live where `io` says (host indices are range-checked, device
 * indices are clamped to [0, S)); `stream` NULL = the null stream of `device`. */
#define QCE_OUT_Y 0
#define QCE_OUT_FEATURES_RAW 1
#define QCE_OUT_FEATURES_DFT 2
int qce_observe_randsnr(const double* h, int64_t B, int N, const double* A, int M, int S, const double* noise_scales,
                        const double* cdf, const int32_t* snr_index_in, int32_t* snr_index_out, int noise_kind,
                        const double* noise, uint64_t seed, uint64_t row_offset, double n_bits,
                        const double* thresholds, const double* labels, int n_levels, int out_kind, void* out,
                        int device, int io, void* stream);

/* out[0] = sum |a_i - b_i|^2 over n complex values (the scripts' MSE numerator, Bussgang_GMM.py:289);
 * deterministic reduction order.  `out` is host memory for QCE_IO_HOST, device memory otherwise. */
int qce_sq_error(const double* a, const double* b, int64_t n, double* out, int device, int io, void* stream);

/* EM training on the device (gmm_cplx_bussgang.py:437-790, `fit_cplx` / `_e_step` / `_m_step`).
 * E-step: the model must be prepared as the fit's channel-domain model (A = NULL, snr_db = +INFINITY,
 * n_bits = +INFINITY: Cr = C).  resp_out (B,K) f64 = exp(log_resp) (:612-656, :676);
 * mean_lse_out[0] = mean_b logsumexp_k lp (the lower bound, :629).  Both where `io` says. */
int qce_em_estep(qce_model* model, const double* X, int64_t B, double* resp_out, double* mean_lse_out, int io,
                 void* stream);

/* M-step `estimate_gaussian_parameters` (:698-737): X (B,N) c128, resp (B,K) f64 ->
 * nk_out (K,) = sum_b resp + 10 eps, means_out (K,N) c128 (zeros when zero_mean), and
 * diag == 0: covs_out (K,N,N) c128 ('full', :739-765); diag != 0: covs_out (K,N) f64 ('diag', :767-790).
 * N <= 256.  Buffers where `io` says (model-free; `stream` NULL = the null stream of `device`). */
int qce_em_mstep(const double* X, int64_t B, int N, int K, const double* resp, double reg_covar, int diag,
                 int zero_mean, double* nk_out, double* means_out, double* covs_out, int device, int io,
                 void* stream);

/* The two weighted statistics of `est_cov_from_quant` (cov_est_quant.py:31-88), for all K components of
 * `estimate_gaussian_covariances_full` / `_inv` (gmm_cplx_quant.py:817, :915) in one pass over X:
 * with d = x_b - means[k] (means (K,N) c128, NULL: d = x_b) and r = resp[b][k] (resp (B,K) f64, NULL: r = 1, K = 1),
 * nk_out (K,) = sum_b r + 10 eps (the M-step's nk),
 * corr_out (K,N,N) c128 = sum_b r s s^H / nk, s = (sign Re d + j sign Im d) / sqrt 2 (:27-28, :45-46; sign(0) = 0),
 * probs_out (K,N,T,2) f64 = sum_b r 1(|Re d_i| < thresholds[t]) / nk, [..][1] the same of Im d_i (:65-69; strict).
 * thresholds: the T positive thresholds of the quantiser, ascending (:60), host memory; T = 0: corr only
 * (probs_out may be NULL).  1 <= N <= 256, 0 <= T <= 15 (beyond: QCE_ENOTIMPL).  X / resp / means / outputs where
 * `io` says (model-free; `stream` NULL = the null stream of `device`); the call returns when the results are written.
 * Deterministic: no atomics, fixed summation order. */
int qce_quant_moments(const double* X, int64_t B, int N, int K, const double* resp, const double* means,
                      const double* thresholds, int T, double* nk_out, double* corr_out, double* probs_out,
                      int device, int io, void* stream);

/* The per-component algebra that follows qce_quant_moments in the quantised M-step, on the device
 * (csrc/qce_quant_recover.hip).  Both calls are model-free, take their buffers where `io` says (`thresholds` is host
 * memory, as above; `stream` NULL = the null stream of `device`), return when the results are written, and are
 * deterministic (no atomics, fixed order).
 *
 * qce_quant_variance_fit: the scalar Gauss-Newton variance fits of `est_cov_from_quant` (cov_est_quant.py:62-84 with
 * utils.py:651-700 `gauss_newt_solve`), one per (component, dimension): probs (K,D,T,2) and nk (K,) as
 * qce_quant_moments returns them, the T >= 1 positive ascending thresholds, the start values x0 (K,D).  p is clipped
 * to [1/nk, (nk-1)/nk]; the 2T residuals are f = erf(t / (sqrt 2 s)) - p with J = -sqrt(2/pi) t exp(-t^2 / (2 s)) / s^2
 * (the reference's exponent); a step is dx = -(J.f)/(J.J) (0 when J.J is exactly 0), until |dx| <= 1e-5 or 100 steps.
 * s2_out (K,D) = max(2 s^2, 0); iters_out (K,D) int32 the steps taken.  The reference restarts a fit whose |s| is
 * below 0.1 or above 10 from numpy's global generator: a fit that reaches either branch, or a non-finite value,
 * stops with status_out (K,D) int32 = 1 (s2_out = 1) and is the caller's to redo; 0 otherwise.
 *
 * qce_herm_eig_clip: out (K,D,D) c128 = V max(L, floor) V^H + diag_post I of the Hermitian A_k = V L V^H, where A_k
 * is C_k (K,D,D) c128 (its lower triangle is read, as eigh reads it) after the element-wise preparation `prep`:
 * QCE_CLIP_PLAIN: C_k; QCE_CLIP_SIN: sin(pi/2 Re C_k) + j sin(pi/2 Im C_k) (the arcsine law);
 * QCE_CLIP_SIN_SCALED: the same times sqrt(s2[k][i] s2[k][j]) (s2 (K,D) f64, else unused); then + diag_pre I.
 * These are the clips of `estimate_gaussian_covariances_full` / `_inv` (gmm_cplx_quant.py:790-800, :819-829,
 * :840-848, :900-920).  Parallel cyclic two-sided Jacobi, one workgroup per component with A and V in LDS; it stops
 * when the off-diagonal Frobenius norm is <= 1e-14 ||A_k||_F.  sweeps_out (K,) int32 the sweeps taken (0: already
 * diagonal); status_out (K,) int32 = 1 for a component still above that bound after 30 sweeps (its `out` is then not
 * to be used), 0 otherwise.  out is exactly Hermitian.  1 <= D <= 64 (beyond: QCE_ENOTIMPL). */
#define QCE_CLIP_PLAIN 0
#define QCE_CLIP_SIN 1
#define QCE_CLIP_SIN_SCALED 2
int qce_quant_variance_fit(const double* probs, const double* nk, const double* thresholds, int T, const double* x0,
                           int K, int D, double* s2_out, int32_t* status_out, int32_t* iters_out, int device, int io,
                           void* stream);
int qce_herm_eig_clip(const double* C, int K, int D, double floor, int prep, const double* s2, double diag_pre,
                      double diag_post, double* out, int32_t* status_out, int32_t* sweeps_out, int device, int io,
                      void* stream);

/* Lloyd's k-means as sklearn's `_kmeans_single_lloyd` runs it (dense data, unit weights): the K-means initialisation
 * of the fits (gmm_cplx_bussgang.py:546-551) without the host.  X (B,N) c128 is clustered as (B, D = 2N) doubles in
 * its stored interleaved order (re0, im0, re1, ...); x_mean (D, NULL = zero) is subtracted from every row as it is
 * loaded.  centers_init / centers_out (K, D): centred, in the same interleaved column order.  The loop stops when no
 * label changed ("strict"), else when the squared centre shift is <= tol_abs, else after max_iter (>= 1) iterations;
 * after a stop that was not strict the rows are assigned once more to the final centres.  Empty clusters take the rows
 * farthest from their centres (`_relocate_empty_clusters_dense`: ascending cluster index, descending distance).
 * labels_out (B,) int64; resp_out (B,K) f64 one-hot (NULL: not wanted);
 * info_out[4] = {n_iter, inertia (sum_b |x_b - c_label(b)|^2), strict (0 / 1), relocated rows}.
 * X / labels_out / resp_out where `io` says; x_mean, both centre arrays and info_out are host memory.
 * 1 <= N <= 256, 1 <= K <= 1024 (beyond: QCE_ENOTIMPL); K > B: QCE_EARG.  Model-free; `stream` NULL = the null stream
 * of `device`; the call returns when the results are written.  Deterministic: no floating-point atomics, fixed
 * summation order. */
int qce_kmeans_lloyd(const double* X, int64_t B, int N, int K, const double* x_mean, const double* centers_init,
                     int max_iter, double tol_abs, double* centers_out, int64_t* labels_out, double* resp_out,
                     double* info_out, int device, int io, void* stream);

/* k-means++ seeding as sklearn's `_kmeans_plusplus` runs it (dense data, unit weights), from random numbers drawn in
 * advance: all its draws are independent of the data (one `choice` for the first centre, `uniform(size=n_trials)` per
 * further centre), so the host draws them in sklearn's order and every step runs on the device.  X and x_mean as for
 * qce_kmeans_lloyd.  first: the row of the first centre.  u (K-1, n_trials), host, each in [0, 1) (NULL allowed when
 * K = 1): for centre c >= 1 the candidates are the first rows whose inclusive cumulative sum of closest[b] (the squared
 * distance to the nearest centre so far) reaches u[c-1][t] * pot (`np.searchsorted`, side "left"; clipped to B - 1),
 * and the candidate with the first smallest new potential becomes the centre (`np.argmin`).  Distances are taken in
 * the difference form.
 * indices_out (K,) int64 the chosen rows; centers_out (K, D) = X[indices] - x_mean (one subtraction per element),
 * centred and interleaved; cand_out (K-1, n_trials) int64 the candidate rows (NULL: not wanted); pot_out (K,) the
 * potential after each centre (NULL: not wanted).  X where `io` says; every other buffer is host memory.
 * 1 <= N <= 256, 1 <= K <= 1024, 1 <= n_trials <= 16 (beyond: QCE_ENOTIMPL); K > B, `first` outside [0, B) or a u
 * outside [0, 1): QCE_EARG.  Model-free; `stream` NULL = the null stream of `device`; all steps are enqueued and the
 * call returns when the results are written.  Deterministic: no floating-point atomics, fixed summation order
 * (csrc/qce_kmeans_seed.hip). */
int qce_kmeans_seed(const double* X, int64_t B, int N, int K, const double* x_mean, int64_t first, const double* u,
                    int n_trials, int64_t* indices_out, double* centers_out, int64_t* cand_out, double* pot_out,
                    int device, int io, void* stream);

/* Set a model option (QCE_OPT_*); drops the prepared state. */
int qce_model_set_option(qce_model* model, int option, double value);

/* Per-sample filters: h_b = W_c y_b + b_c with c = comp[b] (int64, B entries, NULL: c = b, B <= K).
 * The genie Bussgang-LMMSE (estimators/blmmse.py:20-62) is a model with one component per sample
 * (C_b = toeplitz(t_b)^T) estimated this way.  y / comp / h_out where `io` says. */
int qce_estimate_assigned(qce_model* model, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                          void* stream);

/* Bussgang least squares (estimators/LS.py: lstsq(A_eff, y)) with the prepared A_eff of component c = comp[b]
 * (NULL: c = b).  Requires column-orthogonal A_eff (A = NULL or kron(x, I), the scripts' pilot matrices):
 * h_i = sum_m conj(A_eff[m][i]) y_m / sum_m |A_eff[m][i]|^2. */
int qce_estimate_ls(qce_model* model, const double* y, int64_t B, const int64_t* comp, double* h_out, int io,
                    void* stream);

/* Bussgang least squares for a general pilot matrix with full column rank (M >= N): h_b = pinv(A_eff_c) y_b,
 * the same solution as estimators/LS.py:32,47,73 (np.linalg.lstsq(A_eff, y)) for full-rank A_eff.  The
 * pseudo-inverses are formed on the device per call (normal equations, Gauss-Jordan).  M < N -> QCE_ENOTIMPL. */
int qce_estimate_ls_general(qce_model* model, const double* y, int64_t B, const int64_t* comp, double* h_out,
                            int io, void* stream);

/* Toeplitz / block-Toeplitz inverse-EM covariance step (gmm_cplx_bussgang.py:792-826, Barton & Fuhrmann):
 * S (K,N,N) c128 = the M-step's weighted sample covariances WITHOUT reg; F2 (P,N) c128 the partial DFT of
 * `fit` (:143-153); sigma (K,P) f64 in/out.  init != 0 (_initialize, :582-586): sigma = max(Re diag(F2 S F2^H), reg),
 * `model` unused.  init == 0: `model` is prepared on the previous covariances (A = NULL, snr = inf, n_bits = inf:
 * its L^-1 gives Cinv); sigma += sigma^2 Re diag(F2 (Cinv S Cinv - Cinv) F2^H), max reg;
 * covs_out (K,N,N) = F2^H diag(sigma) F2 + reg I.  Host buffers; synchronous. */
int qce_em_toeplitz(qce_model* model, const double* S, int K, int N, const double* F2, int P, double* sigma, double reg,
                    int init, double* covs_out, int device, void* stream);

/* SCM multi-path channels (modules/SCM3GPP/SCMMulti.py:30-56 generate_channel, scm_helper.py:17-84):
 * h_out (B, n_coherence, N) complex64, t_out (B, N) complex64 (first covariance rows).  gains / angles
 * (B, n_path) f64 (normalised gains, angles in degrees) and x (B, 100 N, n_coherence) c128 (the crandn draw)
 * may be supplied — the reference's own draws give its channels to float32 rounding — or NULL: then drawn on the
 * device from Philox4x32-10 keyed by `seed`.  N <= 256, n_path <= 16.  Buffers where `io` says. */
int qce_scm_generate(int64_t B, int n_coherence, int N, int n_path, double path_sigma, const double* gains,
                     const double* angles, const double* x, uint64_t seed, float* h_out, float* t_out, int device,
                     int io, void* stream);

/* Statistical achievable-rate lower bound of the scripts (Bussgang_GMM.py:146-162 and its copies
 * :206-216, :238-249, :291-306): g_b = h_est_b / max(||h_est_b||^2, norm_clip) (norm_clip 0: no clip; the
 * GMM branch uses 0.1), inner_b = g_b^H diag(buss) h_b, den2_b = Re g_b^H Cq g_b;
 * out[0] = log2(1 + num / (den1 + den2)), out[1] = num = |mean inner|^2, out[2] = den1 = var(inner),
 * out[3] = den2 = mean den2_b.  h_est / h (B,N) c128 where `io` says; buss (N,) f64, Cq (N,N) c128 and out
 * host; synchronous. */
int qce_rate_bound(const double* h_est, const double* h, int64_t B, int N, const double* buss, const double* Cq,
                   double norm_clip, double* out, int device, int io, void* stream);

/* Per-sample matched-filter rate of the scripts' LS branch (Bussgang_GMM.py:186-198): g = (buss o h_est_b)^H Cq^-1,
 * out[0] = mean_b Re log2(1 + |g B h_est_b|^2 / (g Cq g^H + |g B (h_b - h_est_b)|^2)), B = diag(buss).  Cq^-1 is
 * formed on the device (Cq Hermitian, full rank: equal to np.linalg.pinv to rounding).  h_est / h (B,N) c128
 * where `io` says; buss (N,) f64, Cq (N,N) c128 and out host; N <= 256; synchronous. */
int qce_rate_mf(const double* h_est, const double* h, int64_t B, int N, const double* buss, const double* Cq,
                double* out, int device, int io, void* stream);

/* VAE-parameterised Bussgang LMMSE (estimators/vae.py:376-431 convert_dec_outputs with zeromean=True, then
 * :368-369 lmmse), model-free: per sample the decoder's log-variances logvar (B,N) (float when logvar_is_f32,
 * else double) give the circulant Ch = F^H diag(max(exp(-logvar), 1e-12)) F; with the pilot matrix
 * A = kron(x, I_N), x_cplx (P,) c128 host array, the conversion and the LMMSE run in the Fourier domain (N-point
 * transforms and a P x P Cholesky per DFT bin, csrc/qce_vae.hip).  y (B, P N) c128 pilot-major -> h_out (B,N) c128.
 * n_bits: 1, 2..16 (uniform quantiser) or +INFINITY.  N: a power of two in [16, 256], P <= 4, else QCE_ENOTIMPL.
 * logvar / y / h_out where `io` says; B of any size (chunked internally); `stream` NULL = the null stream of
 * `device`.  The call synchronises the stream to read the status: QCE_ECHOL if some bin's P x P matrix is not
 * positive definite (the reference's pinv is not emulated). */
int qce_vae_estimate(int N, int P, const double* x_cplx, double snr_db, double n_bits, const void* logvar,
                     int logvar_is_f32, const double* y, int64_t B, double* h_out, int io, int device, void* stream);

/* The VAE estimator's inference network in one kernel (estimators/vae.py:161-172 and :294-309 forward_nosamp;
 * csrc/qce_vae_net.hip): features (unitary DFT in FP64, rounded once to float32), the pilot convolutions (kernel
 * size 1), the encoder up to the latent mean and the decoder, float32 on v_mfma_f32_16x16x4_f32.
 *
 * qce_vae_net_create: `widths` (host) holds the convolutions' channel counts (n_pilot_convs + 1 entries, P .. 1), the
 * encoder's widths (n_layers + 1, 2N .. 2L) and the decoder's (n_layers + 1, L .. N).  `weights` is one flat float32
 * buffer (host or device memory, as `io` says) in the reference's state-dict order: the convolutions, the encoder's
 * layers, the decoder's; each layer its weight (out, in) row-major, then its bias.  The library keeps a copy and a
 * zero-padded repacking.  genie != 0: the network encodes the true channel (one row, always transformed, no
 * convolutions applied).  Refused before any device call: QCE_ENOTIMPL for N not a power of two in [16, 256], P > 4,
 * L outside [1, 128], n_layers outside [1, 8], n_pilot_convs > 4, a width above 512; QCE_EARG for inconsistent widths,
 * P > 1 without convolutions on a non-genie network, n_weights other than the widths imply, a NULL pointer.
 *
 * qce_vae_net_forward: net_in (B, P N) c128 observations, pilot-major, or (B, N) true channels for a genie network;
 * fft_pre == 0 takes [Re | Im] of the observations untransformed.  mu_out (B, L) and logvar_out (B, N) float32 may be
 * NULL.  With h_out (B, N) c128 non-NULL the call continues on the same stream into the LMMSE of qce_vae_estimate with
 * y (B, P N), x_cplx, snr_db and n_bits as there (chunks of 65536 rows, two launches per chunk; the log-variances stay
 * in a scratch of one chunk that the handle owns when logvar_out is NULL), synchronises the stream and returns
 * QCE_ECHOL as qce_vae_estimate does.  Without h_out and with device buffers the call is asynchronous.  Buffers where
 * `io` says; `stream` NULL = the null stream of the handle's device.  A handle serves one call at a time.
 * A row's result does not depend on B or on its place in the batch. */
typedef struct qce_vae_net qce_vae_net;
int qce_vae_net_create(int N, int P, int L, int n_layers, int n_pilot_convs, int genie, const int32_t* widths,
                       const float* weights, int64_t n_weights, int io, int device, qce_vae_net** out);
int qce_vae_net_forward(qce_vae_net* net, const double* net_in, int fft_pre, int64_t B, float* mu_out, float* logvar_out,
                        const double* y, const double* x_cplx, double snr_db, double n_bits, double* h_out, int io,
                        void* stream);
int qce_vae_net_destroy(qce_vae_net* net);

/* Training side of the VAE estimator (estimators/vae.py:280-281 and :312-365 vae_loss; csrc/qce_vae_train.hip),
 * model-free.  All buffers are device memory (QCE_IO_DEVICE only), all three calls are asynchronous on `stream`
 * (NULL = the null stream of `device`) and leave no status to read; refusals come before any launch.
 * enc (B, 2L) float32 = [mu | s] is the encoder output (s = log_var_enc), 1 <= L <= 128 (more: QCE_ENOTIMPL).
 *
 * qce_vae_sample: z = mu + exp(s) eps -> z_out (B, L) float32, FP64 arithmetic rounded once.  eps_in (B, L) float32, or
 * NULL: eps drawn on the device (Philox4x32-10 keyed by seed, a stream of its own; element (b, l) uses counter
 * (row_offset + b) L + l, so rows [B1, B) generated with row_offset = B1 equal the one-shot rows).  eps_out (B, L)
 * receives the eps used (may be NULL when eps_in is given).
 * qce_vae_sample_bwd: grad_enc (B, 2L) = [grad_z | grad_z exp(s) eps]. */
int qce_vae_sample(const float* enc, int64_t B, int L, const float* eps_in, uint64_t seed, uint64_t row_offset,
                   float* z_out, float* eps_out, int device, void* stream);
int qce_vae_sample_bwd(const float* enc, const float* eps, const float* grad_z, int64_t B, int L, float* grad_enc,
                       int device, void* stream);

/* qce_vae_elbo: rows_out[b] = the row ELBO l_b (float64) of vae_loss with zeromean=True, and in the same pass the
 * gradient of the loss -mean_b l_b: grad_dec (B, N) float32 with respect to dec, grad_enc (B, 2L) float32 the direct
 * (KL) part with respect to enc, both including the factor 1 / B.  dec (B, N) float32 = log_var_dec; target
 * (n_target, 2N) float32 = [re | im]; row b uses target row index[b] (int32, clamped to [0, n_target)), or row b when
 * index is NULL (then n_target >= B).  mode 0: 'genie' / 'noisy' (n_bits, snr_db ignored).  mode 1: 'real' with a
 * uniform quantiser of n_bits in 1..8 or +INFINITY (none) and snr_db (n_target,) float64, row b at snr_db[index[b]].
 * N: a power of two in [16, 256], else QCE_ENOTIMPL.  dec, target and grad_dec 16-byte aligned.  Equal inputs give
 * bit-identical outputs (no atomics; the mean over rows is the caller's). */
int qce_vae_elbo(const float* enc, const float* dec, const float* target, int64_t n_target, int64_t B, int N, int L,
                 int mode, double n_bits, const int32_t* index, const double* snr_db, double* rows_out,
                 float* grad_enc, float* grad_dec, int device, void* stream);

/* The fused training step (csrc/qce_vae_step.hip): a trainer owns the weights, Adam's two moments and its step count
 * on the device, and runs one training step of the reference's loop (estimators/vae.py:108-123) as two kernels:
 * k_vae_step (gather the batch by index, pilot convolutions, encoder, z = mu + exp(s) eps, decoder, the row ELBO of
 * qce_vae_elbo, the backward pass, one partial gradient per tile of 16 rows) and k_vae_update (sum of the partials in
 * tile order, loss = -mean_b l_b in FP64, skip rule, torch's default Adam).  Equal state and inputs give bit-identical
 * results.
 *
 * qce_vae_trainer_create: mode 0 'genie' (x is (n_x, 2N), the convolutions are not applied), 1 'noisy', 2 'real';
 * widths as qce_vae_net_create; weights (n_weights,) float32 in state-dict order, host memory (QCE_IO_HOST) or
 * device memory (QCE_IO_DEVICE); max_batch bounds B of later calls.  Refused with QCE_ENOTIMPL before any device call:
 * N outside {16, 32, 64, 128}, P > 4, L > 128, and a network whose LDS need (the stored activations of 16 rows, two
 * delta buffers and staging; the message states it) exceeds 160 KiB.
 * qce_vae_trainer_step: one step; all pointers device memory, asynchronous on `stream`, no status read.  x (n_x, P, 2N)
 * float32 features, target (n_target, 2N) float32, snr_db (n_target,) float64 ('real' only), index (B,) int32 rows of x
 * and target (clamped; NULL: row b), n_bits as qce_vae_elbo ('real' only), eps (B, L) float32 or NULL: drawn as
 * qce_vae_sample draws it from (seed, row_offset).  The loss goes to slot step_slot (< QCE_VAE_TRAINER_SLOTS) of the
 * trainer's loss record together with a flag: 1 when the loss was NaN or above 1000, and then weights, moments and
 * step count are left untouched.
 * qce_vae_trainer_grads: the same forward, loss and backward without an update: grads_out (n_weights,) float32,
 * rows_out (B,) float64 row ELBOs, loss_out one float64; device memory, asynchronous.
 * qce_vae_trainer_read: the first n slots of the loss record into host arrays; synchronises `stream`.
 * qce_vae_trainer_get_state / _set_state: weights, exp_avg, exp_avg_sq (device memory, each may be NULL) and the step
 * count (host); both synchronise `stream`. */
#define QCE_VAE_TRAINER_SLOTS 4096
typedef struct qce_vae_trainer qce_vae_trainer;
int qce_vae_trainer_create(int N, int P, int L, int n_layers, int n_pilot_convs, int mode, const int32_t* widths,
                           const float* weights, int64_t n_weights, double lr, int64_t max_batch, int io, int device,
                           qce_vae_trainer** out);
int qce_vae_trainer_step(qce_vae_trainer* tr, const float* x, int64_t n_x, const float* target, int64_t n_target,
                         const double* snr_db, const int32_t* index, int64_t B, double n_bits, const float* eps,
                         uint64_t seed, uint64_t row_offset, int step_slot, void* stream);
int qce_vae_trainer_grads(qce_vae_trainer* tr, const float* x, int64_t n_x, const float* target, int64_t n_target,
                          const double* snr_db, const int32_t* index, int64_t B, double n_bits, const float* eps,
                          uint64_t seed, uint64_t row_offset, float* grads_out, double* rows_out, double* loss_out,
                          void* stream);
int qce_vae_trainer_read(qce_vae_trainer* tr, double* losses_out, int32_t* skipped_out, int n, void* stream);
int qce_vae_trainer_get_state(qce_vae_trainer* tr, float* weights_out, float* exp_avg_out, float* exp_avg_sq_out,
                              int64_t* step_out, void* stream);
int qce_vae_trainer_set_state(qce_vae_trainer* tr, const float* weights, const float* exp_avg, const float* exp_avg_sq,
                              int64_t step, void* stream);
int qce_vae_trainer_destroy(qce_vae_trainer* tr);

/* Page-locked host memory (hipHostMalloc / hipHostFree).  QCE_IO_HOST calls DMA straight from / into page-locked
 * arrays (and from / into pageable ones they can register for the call): a caller that allocates its result arrays
 * here, and reuses them, saves the page faults of fresh pageable memory (the Python layer's result pool, _lib.py). */
int qce_host_alloc(size_t bytes, void** out);
int qce_host_free(void* p);

/* Device synchronisation of the model's stream (for timing and for QCE_IO_DEVICE callers). */
int qce_synchronize(qce_model* model);

/* ---------------------------------------------------------------------------------------------------------------
 * K-shard estimation over a communicator.  Replaces the reference's only parallelism,
 * a process pool over SNR points (Bussgang_GMM.py:29-32, :287), by one process per GPU, each holding a contiguous
 * slice of the mixture's components (qce_kshard_slice), with the collectives issued by the library itself:
 * RCCL (ncclAllReduce / ncclReduceScatter / ncclAllGather over xGMI) or a caller-supplied host transport.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct qce_comm qce_comm;
typedef struct qce_kshard qce_kshard;

#define QCE_COMM_ID_BYTES 128 /* ncclUniqueId */
#define QCE_COMM_RCCL 0
#define QCE_COMM_HOST 1

/* collective ops of a host transport; all data are doubles */
#define QCE_COLL_ALLREDUCE_SUM 0 /* recv[i] = sum_r send_r[i], count elements                          */
#define QCE_COLL_ALLREDUCE_MAX 1 /* recv[i] = max_r send_r[i], count elements                          */
#define QCE_COLL_REDUCE_SCATTER_SUM 2 /* send: world * count, recv[i] = sum_r send_r[rank * count + i]  */
#define QCE_COLL_ALLGATHER 3     /* send: count, recv[r * count + i] = send_r[i]                      */

/* A host transport (MPI, gloo, ...): called synchronously with host buffers (the library has synchronised the
 * stream and staged the device data); returns 0 on success. */
typedef int (*qce_host_collective)(void* user, int op, const double* send, double* recv, int64_t count);

/* ncclGetUniqueId: called on one rank, the QCE_COMM_ID_BYTES bytes are then shared with every rank. */
int qce_comm_unique_id(void* id_out);
/* ncclCommInitRank on `device` (collective over the `world` ranks). */
int qce_comm_init(const void* unique_id, int rank, int world, int device, qce_comm** out);
/* A communicator whose collectives go through the caller's host transport `fn` (`user` passed through). */
int qce_comm_init_host(int rank, int world, int device, qce_host_collective fn, void* user, qce_comm** out);
int qce_comm_destroy(qce_comm* comm);
int qce_comm_info(qce_comm* comm, int* rank, int* world, int* device, int* kind);

/* Components [lo, hi) of rank `rank` in the balanced contiguous split of K over `world` ranks (K >= world). */
int qce_kshard_slice(int K, int world, int rank, int* lo, int* hi);
/* (world, rank) a K-shard's rows are laid out for: the communicator's, or on a world-1 communicator the test hook
 * QCE_KSHARD_EMULATE_WORLD="W[:R]" (2 <= W <= 4096, 0 <= R < W; anything else is ignored) that qce_kshard_create
 * applies.  Host-only: needs no GPU. */
int qce_kshard_layout(int world, int rank, int* layout_world, int* layout_rank);
/* Rows of h_out a rank receives from qce_kshard_estimate: per pipeline chunk the global row range
 * [ranges[2i], ranges[2i+1]) (concatenated in h_out in this order); scatter = 0: every rank gets all B rows.
 * `cap` = number of ranges the array holds; *n = ranges written.  Selective modes use chunks = 1. */
int qce_kshard_rows(int64_t B, int chunks, int world, int rank, int scatter, int64_t* ranges, int cap, int* n);

/* A K-shard estimator: `shard` holds components qce_kshard_slice(K_total, world, rank) of the mixture (a model
 * created from that slice), `comm` its communicator.  Neither is owned. */
int qce_kshard_create(qce_model* shard, qce_comm* comm, int K_total, qce_kshard** out);
int qce_kshard_destroy(qce_kshard* ks);
/* Double-buffered tables: `spare` is a second model of the same shard (same parameters; not owned).  Prepares then
 * alternate between the two table sets on the library's prepare stream: prepare t+1 waits only for the last step
 * that read its set (step t-1), so it runs beside step t's partial kernels (Bussgang_GMM.py:284-287: the next SNR
 * point's tables do not depend on the current estimate).  A prepare issues no collective. */
int qce_kshard_set_spare(qce_kshard* ks, qce_model* spare);
/* Per-SNR prepare of the shard (qce_prepare) and the shard's shift M_r = max over its components of
 * c_k = -M log(pi) + 2 log det P_k + log w_k (>= every local lp: the quad form is >= 0; +inf when a Cholesky
 * factorisation failed).  No collective and no host synchronisation: the shards agree on M* = max_r M_r at the start
 * of the next qce_kshard_estimate, on the library's communication stream. */
int qce_kshard_prepare(qce_kshard* ks, const double* A, int M, double snr_db, double n_bits, int quant_kind,
                       const double* thresholds, const double* labels, int n_levels, void* stream);
/* One estimate step over y (B, M) c128 in device memory (the same y on every rank).  Its first collective is an
 * 8-byte MAX of the shards' shifts M_r (M*); every collective of the library is issued on one communicator from its
 * communication stream, so all ranks issue them in the same order.
 * QCE_MODE_ALL (gmm_cplx_bussgang.py:220-228): per chunk the shard's FP64 partial rows [s e^{m-M_r}, 0,
 * acc e^{m-M_r}] (qce_estimate_partial_shifted) and one SUM collective of them on the communication stream
 * (reduce-scatter, scatter != 0, or all-reduce) that scales each shard's rows by e^{M_r - M*} on the way in (RCCL
 * PreMulSum, scalar in device memory), overlapped with the next chunk's kernel; h = acc / s.  QCE_MODE_TOPN / QCE_MODE_CUMP (:197-219, :229-242): n == 1 all-gathers each shard's (max lp, index)
 * and the owner of the first global maximum contributes W_j y + b_j; otherwise the shards' lp are all-gathered,
 * every rank selects the same components (k_select on the full lp) and the shards' weighted filter sums are
 * summed (one chunk).  h_out: device memory, the rows qce_kshard_rows names.  A 2-double MAX of the step's flag
 * word [rows whose shifted sum underflowed, Cholesky failure on any rank] closes the step; nothing is read on the
 * host until qce_kshard_finish.  The step's collectives and row finalisation run on the library's communication
 * stream and may still be in flight when the next step's kernels start on `stream` (the send rows alternate between
 * two buffers); h_out is complete once qce_kshard_finish returned, which also orders `stream` after the step.  y and
 * every h_out since the last finish must stay valid until then. */
int qce_kshard_estimate(qce_kshard* ks, const double* y, int64_t B, int mode, double mode_param, int chunks,
                        int scatter, double* h_out, void* stream);
/* The caller's sync point: reads the flag words (one host synchronisation).  QCE_ECHOL with the reference's
 * message (gmm_cplx_bussgang.py:43-46) if a Cholesky factorisation failed on any rank -- on every rank; rows of
 * the last step whose shifted sum underflowed are recombined exactly (collective: per-row MAX of the shards'
 * running maxima, then the SUM); QCE_ESTATE if an earlier, already superseded step had such rows. */
int qce_kshard_finish(qce_kshard* ks, void* stream);
/* The flag words the last qce_kshard_finish read: [rows of the last step recombined exactly, Cholesky failure on
 * some rank, the same two for the superseded steps before it] (diagnostics and tests). */
int qce_kshard_flags(qce_kshard* ks, double* out4);
/* Kernel timing of the shard's estimate launches (HIP events around each partial / lp launch on the compute
 * stream): enable != 0 starts recording (clears earlier records); qce_kshard_kernel_ms synchronises on the
 * recorded events, returns their summed duration and count, and clears them. */
int qce_kshard_timing(qce_kshard* ks, int enable);
int qce_kshard_kernel_ms(qce_kshard* ks, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* QCE_H */
