// Private header of the C-ABI host units (qce_capi*.hip, qce_kshard.hip, qce_big.hip): the error slot, the HIP
// check macro and the device guard they all use, then the helpers the qce_capi*.hip units share.
#pragma once
#include <string>
#include <vector>

#include "../../include/qce.h"
#include "qce_kernels.h"
#include "qce_model.h"

int qce_set_error(int code, const std::string& msg);  // sets qce_last_error() and returns code

#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return qce_set_error(QCE_EHIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));    \
  } while (0)

// Makes `dev` the calling thread's device for one C-ABI call and puts the caller's back at its end.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev && hipSetDevice(dev) != hipSuccess) (void)hipGetLastError();  // no sticky error left behind
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// stream-ordered scratch for the model-free entry points (freed on the same stream)
struct StreamScratch {
  hipStream_t st;
  std::vector<void*> ptrs;
  explicit StreamScratch(hipStream_t s) : st(s) {}
  hipError_t get(void** p, size_t bytes) {
    hipError_t e = hipMallocAsync(p, bytes ? bytes : 1, st);
    if (e == hipSuccess) ptrs.push_back(*p);
    return e;
  }
  ~StreamScratch() {
    for (void* p : ptrs) (void)hipFreeAsync(p, st);
  }
};

// ---------------------------------------------------------------------------------------------------------------
// shared by the qce_capi*.hip units
// ---------------------------------------------------------------------------------------------------------------
inline hipStream_t pick_stream(qce_model* m, void* stream) { return stream ? (hipStream_t)stream : m->stream; }

// qce_capi_prepare.hip
hipError_t detect_structure(qce_model* m);  // at creation / set_params: is the mixture (block-)circulant?
int check_status(qce_model* m, bool block);  // the last prepare's Cholesky status, once it is known (block: wait)
int check_model(qce_model* m, bool need_prepared);
int ensure_dense(qce_model* m, void* stream = nullptr);  // dense tables of a prepare that took the Fourier path
double uniform_std_step(int nb);  // the unit-variance step of uniform_quantizer.py:6-21
double uniform_step(double snr_db, int nb);

#define HOST_SYNC_CHECK(m, st)                         \
  do {                                                 \
    HIPCHK(hipStreamSynchronize(st));                  \
    if (int rc_ = check_status((m), true)) return rc_; \
  } while (0)

// qce_capi_estimate.hip
// Arithmetic of the dense 'all' / partial path for this model: the model option, overridden by
// QCE_KERNEL=f64 | h2 | f32 (A/B runs).
bool want_f64(const qce_model* m);
// The model asks for the int8 family (QCE_PRECISION_INT8 and no QCE_KERNEL override); select_backend grants it where
// the quantiser and the shape allow, and falls back to the f64 families elsewhere.
bool want_int8(const qce_model* m);
// FP64 raw sums of one component on the int8 kernel (qce_debug_i8_products)
int run_i8_debug(qce_model* m, const double2* dy, long long B, int k, double* rawL, double* rawW, hipStream_t st);
QceFftEstArgs fft_args(qce_model* m, const double2* y, long long B);
// stage host input (io == HOST) or use the device pointer directly
int stage_input(qce_model* m, const double* y, long long B, int io, hipStream_t st, const double2** dy);
// lp (B x K) of the prepared model on the family's log-prob kernel
int backend_lp(qce_model* m, const double2* x, long long B, double* lp, hipStream_t st);

// qce_capi_free.hip
// the constants of k_vae for one (snr, n_bits, pilot vector), shared by qce_vae_estimate and qce_vae_net_forward
int vae_lmmse_args(const char* who, int N, int P, const double* x_cplx, double snr_db, double n_bits, QceVaeArgs* a);

#ifdef QCE_STAMPS
// qce_capi_debug.hip (diagnostic build): segment cycles of the last FP64 launch
extern unsigned long long* g_f64_stamps;
extern long long g_f64_stamp_records;
#endif

// qce_capi_hostio.hip
// rows per host-pipeline chunk; 0 = one shot (QCE_HOST_PIPELINE=0, or too small a batch to split)
long long host_chunk_rows(const qce_model* m, long long B);
int estimate_host_chunked(qce_model* m, const double* y, long long B, long long C, int mode, double mode_param,
                          double* h_out, hipStream_t st);
