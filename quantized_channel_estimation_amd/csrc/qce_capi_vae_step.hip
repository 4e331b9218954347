// C ABI of libqce.so, the fused VAE training step (qce_vae_step.hip): a trainer that owns the weights, Adam's moments
// and step count, the per-tile partial gradients and the loss record on the device.  Every refusal of
// qce_vae_trainer_create happens before a device call; the step itself is asynchronous and reads no status.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qce_capi.h"
#include "qce_common.h"

struct qce_vae_trainer {
  int N, P, L, mode, device;
  int64_t max_batch, n_params;
  double lr;
  QceVaeStepArgs proto;  // everything but the batch
  float *w = nullptr, *m = nullptr, *v = nullptr, *partials = nullptr;
  double *rows = nullptr, *losses = nullptr;  // losses: QCE_VAE_TRAINER_SLOTS, then one scratch entry
  int* skipped = nullptr;
  long long* count = nullptr;  // [0] Adam's step count, [1] the copy k_vae_step hands to k_vae_update
};

namespace {

int up16i(int v) { return (v + 15) & ~15; }

std::string tr_err(const std::string& msg) { return "vae_trainer_create: " + msg; }

void release(qce_vae_trainer* t) {
  void* ptrs[] = {t->w, t->m, t->v, t->partials, t->rows, t->losses, t->skipped, t->count};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete t;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// The batch part of the arguments, checked; *a is the trainer's prototype filled in.
int batch_args(const char* who, qce_vae_trainer* tr, const float* x, int64_t n_x, const float* target, int64_t n_target,
               const double* snr_db, const int32_t* index, int64_t B, double n_bits, const float* eps, uint64_t seed,
               uint64_t row_offset, QceVaeStepArgs* a) {
  const std::string w(who);
  if (!tr) return qce_set_error(QCE_EARG, w + ": null handle");
  if (B < 1 || B > tr->max_batch)
    return qce_set_error(QCE_EARG, w + ": the batch must lie in [1, max_batch = " + std::to_string(tr->max_batch) + "]");
  if (!x || !target) return qce_set_error(QCE_EARG, w + ": null buffer");
  if (index ? (n_x < 1 || n_target < 1) : (n_x < B || n_target < B))
    return qce_set_error(QCE_EARG, w + ": x or target has fewer rows than the batch uses");
  if (misaligned(x) || misaligned(target)) return qce_set_error(QCE_EARG, w + ": x and target must be 16-byte aligned");
  *a = tr->proto;
  if (tr->mode == 2) {
    if (isinf(n_bits) && n_bits > 0) a->n_bits = 0;
    else {
      a->n_bits = (int)n_bits;
      if (!(n_bits >= 1.0) || (double)a->n_bits != n_bits)
        return qce_set_error(QCE_EARG, w + ": n_bits must be an integer >= 1 or inf");
      if (a->n_bits > 8) return qce_set_error(QCE_ENOTIMPL, w + ": the 'real' loss covers uniform quantisers up to 8 bits");
      a->step = uniform_std_step(a->n_bits);
    }
    if (!snr_db) return qce_set_error(QCE_EARG, w + ": mode 'real' needs snr_db");
  }
  a->B = B;
  a->n_x = n_x;
  a->T = n_target;
  a->x = x;
  a->t = target;
  a->index = index;
  a->snr = tr->mode == 2 ? snr_db : nullptr;
  a->eps = eps;
  a->seed = seed;
  a->row_offset = row_offset;
  return QCE_OK;
}

QceVaeUpdateArgs update_args(const qce_vae_trainer* tr, int64_t B) {
  QceVaeUpdateArgs u{};
  u.B = B;
  u.tiles = (int)((B + QCE_VAE_NET_ROWS - 1) / QCE_VAE_NET_ROWS);
  u.n_params = (int)tr->n_params;
  u.partials = tr->partials;
  u.rows = tr->rows;
  u.count_snap = tr->count + 1;
  u.count = tr->count;
  u.lr = tr->lr;
  return u;
}

}  // namespace

extern "C" {

int qce_vae_trainer_create(int N, int P, int L, int n_layers, int n_pilot_convs, int mode, const int32_t* widths,
                           const float* weights, int64_t n_weights, double lr, int64_t max_batch, int io, int device,
                           qce_vae_trainer** out) {
  if (!widths || !weights || !out) return qce_set_error(QCE_EARG, tr_err("null pointer"));
  *out = nullptr;
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, tr_err("bad io"));
  if (mode < 0 || mode > 2) return qce_set_error(QCE_EARG, tr_err("mode must be 0 (genie), 1 (noisy) or 2 (real)"));
  if (P < 1 || n_pilot_convs < 0 || max_batch < 1 || max_batch > 0x7fffffffLL || !(lr > 0.0))
    return qce_set_error(QCE_EARG, tr_err("bad shape"));
  if (N == 256)
    return qce_set_error(QCE_ENOTIMPL, tr_err("n_antennas = 256 is not covered by the fused step: the activations of 16 rows "
                                              "do not fit the LDS of one workgroup"));
  if (N != 16 && N != 32 && N != 64 && N != 128)
    return qce_set_error(QCE_ENOTIMPL, tr_err("n_antennas must be 16, 32, 64 or 128, got " + std::to_string(N)));
  if (P > QCE_VAE_MAX_PILOTS)
    return qce_set_error(QCE_ENOTIMPL, tr_err("at most " + std::to_string(QCE_VAE_MAX_PILOTS) + " pilots, got " + std::to_string(P)));
  if (L < 1 || L > QCE_VAE_MAX_LATENT)
    return qce_set_error(QCE_ENOTIMPL, tr_err("latent_dim must lie in [1, " + std::to_string(QCE_VAE_MAX_LATENT) + "], got " +
                                              std::to_string(L)));
  if (n_layers < 1 || n_layers > QCE_VAE_NET_MAX_LAYERS)
    return qce_set_error(QCE_ENOTIMPL, tr_err("n_layers must lie in [1, " + std::to_string(QCE_VAE_NET_MAX_LAYERS) + "], got " +
                                              std::to_string(n_layers)));
  if (n_pilot_convs > QCE_VAE_NET_MAX_CONVS)
    return qce_set_error(QCE_ENOTIMPL, tr_err("at most " + std::to_string(QCE_VAE_NET_MAX_CONVS) + " pilot convolutions, got " +
                                              std::to_string(n_pilot_convs)));
  const int32_t* conv = widths;
  const int32_t* enc = conv + n_pilot_convs + 1;
  const int32_t* dec = enc + n_layers + 1;
  const int nw = n_pilot_convs + 1 + 2 * (n_layers + 1);
  for (int i = 0; i < nw; ++i) {
    if (widths[i] < 1) return qce_set_error(QCE_EARG, tr_err("widths must be positive"));
    if (widths[i] > QCE_VAE_NET_MAX_WIDTH)
      return qce_set_error(QCE_ENOTIMPL, tr_err("layer widths up to " + std::to_string(QCE_VAE_NET_MAX_WIDTH) + ", got " +
                                                std::to_string(widths[i])));
  }
  const bool genie = mode == 0;
  if (P > 1 && n_pilot_convs == 0 && !genie)
    return qce_set_error(QCE_EARG, tr_err("several pilots need n_pilot_convs >= 1 (the encoder takes one row)"));
  if (mode == 2 && P > 1) return qce_set_error(QCE_ENOTIMPL, tr_err("mode 'real' trains with one pilot"));
  if (conv[0] != P || (n_pilot_convs > 0 && conv[n_pilot_convs] != 1) || enc[0] != 2 * N || enc[n_layers] != 2 * L ||
      dec[0] != L || dec[n_layers] != N)
    return qce_set_error(QCE_EARG, tr_err("inconsistent widths: conv P .. 1, enc 2N .. 2L, dec L .. N"));
  for (int i = 0; i <= n_pilot_convs; ++i)
    if (conv[i] > QCE_VAE_MAX_PILOTS)
      return qce_set_error(QCE_ENOTIMPL, tr_err("pilot convolutions of up to " + std::to_string(QCE_VAE_MAX_PILOTS) + " channels"));

  QceVaeStepArgs a;
  memset(&a, 0, sizeof(a));
  a.N = N;
  a.L = L;
  a.mode = mode == 2 ? 1 : 0;
  a.sqrt_pi_f = sqrtf((float)M_PI);  // torch.sqrt(torch.tensor(torch.pi, dtype=torch.float)), uniform_quantizer.py:110
  a.nconv = genie ? 0 : n_pilot_convs;
  a.P = a.nconv ? P : 1;
  int64_t off = 0;
  for (int i = 0; i < n_pilot_convs; ++i) {  // (a genie network carries the convolutions' weights and never uses them)
    a.conv_ch[i] = conv[i];
    a.conv_off[i] = (int)off;
    off += (int64_t)conv[i + 1] * conv[i] + conv[i + 1];
  }
  a.conv_ch[n_pilot_convs] = conv[n_pilot_convs];
  const int64_t n_conv = off;
  a.n_conv_params = a.nconv ? (int)n_conv : 0;
  a.nenc = n_layers;
  a.nlayers = 2 * n_layers;
  // LDS: one buffer per stored activation (16 rows, stride = width rounded up to 16, + 4)
  int64_t lds = 0;
  int widest = 2 * N;
  auto buffer = [&](int width, int* at, int* stride) {
    *stride = up16i(width) + 4;
    *at = (int)lds;
    lds += (int64_t)QCE_VAE_NET_ROWS * *stride;
    if (width > widest) widest = width;
  };
  int at = 0, stride = 0;
  buffer(2 * N, &at, &stride);
  for (int half = 0; half < 2; ++half) {
    const int32_t* wd = half ? dec : enc;
    if (half) buffer(L, &at, &stride);  // z
    for (int i = 0; i < n_layers; ++i) {
      QceVaeStepLayer* ly = &a.layer[half * n_layers + i];
      ly->in = wd[i];
      ly->out = wd[i + 1];
      ly->w_off = (int)off;
      ly->b_off = (int)(off + (int64_t)wd[i + 1] * wd[i]);
      off += (int64_t)wd[i + 1] * wd[i] + wd[i + 1];
      ly->relu = i < n_layers - 1;
      ly->src = at;
      ly->s_src = stride;
      buffer(wd[i + 1], &at, &stride);
      ly->dst = at;
      ly->s_dst = stride;
    }
  }
  const int64_t act_floats = lds;
  a.red_off = 0;  // the convolutions' reduction staging takes the activations' place once they are dead
  if ((int64_t)a.n_conv_params * 256 > lds) lds = (int64_t)a.n_conv_params * 256;
  a.x_off = (int)lds;
  if (a.nconv) lds += (int64_t)QCE_VAE_NET_ROWS * a.P * 2 * N;
  a.eps_off = (int)lds;
  lds += (int64_t)QCE_VAE_NET_ROWS * L;
  a.kl_off = (int)lds;
  lds += (int64_t)QCE_VAE_NET_ROWS * 2 * L;
  a.s_delta = up16i(widest) + 4;
  a.d0_off = (int)lds;
  lds += (int64_t)QCE_VAE_NET_ROWS * a.s_delta;
  a.d1_off = (int)lds;
  lds += (int64_t)QCE_VAE_NET_ROWS * a.s_delta;
  const int64_t row_table = 2 * sizeof(long long) * QCE_VAE_NET_ROWS;  // the kernel's static gather table
  const int64_t need = 4 * lds + row_table;
  if (need > QCE_VAE_STEP_LDS_LIMIT)
    return qce_set_error(QCE_ENOTIMPL,
                         tr_err("this network needs " + std::to_string(need) + " bytes of LDS per workgroup (" +
                                std::to_string(4 * act_floats) + " of stored activations of 16 rows, " +
                                std::to_string(8 * QCE_VAE_NET_ROWS * a.s_delta) + " of two delta buffers, " +
                                std::to_string(need - 4 * act_floats - 8 * QCE_VAE_NET_ROWS * a.s_delta) +
                                " of staging); the fused step covers up to " + std::to_string(QCE_VAE_STEP_LDS_LIMIT)));
  if (n_weights != off)
    return qce_set_error(QCE_EARG, tr_err("the widths imply " + std::to_string(off) + " weights, got " + std::to_string(n_weights)));
  a.lds_bytes = (unsigned)(4 * lds);
  a.n_params = (int)off;

  DeviceGuard g(device);
  qce_vae_trainer* t = new qce_vae_trainer();
  t->N = N;
  t->P = P;
  t->L = L;
  t->mode = mode;
  t->device = device;
  t->max_batch = max_batch;
  t->n_params = off;
  t->lr = lr;
  const size_t wb = sizeof(float) * (size_t)off;
  const size_t tiles = (size_t)((max_batch + QCE_VAE_NET_ROWS - 1) / QCE_VAE_NET_ROWS);
  hipError_t e = hipMalloc((void**)&t->w, wb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->m, wb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->v, wb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->partials, wb * tiles);
  if (e == hipSuccess) e = hipMalloc((void**)&t->rows, sizeof(double) * (size_t)max_batch);
  if (e == hipSuccess) e = hipMalloc((void**)&t->losses, sizeof(double) * (QCE_VAE_TRAINER_SLOTS + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&t->skipped, sizeof(int) * QCE_VAE_TRAINER_SLOTS);
  if (e == hipSuccess) e = hipMalloc((void**)&t->count, 2 * sizeof(long long));
  if (e == hipSuccess) e = hipMemcpy(t->w, weights, wb, io == QCE_IO_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(t->m, 0, wb);
  if (e == hipSuccess) e = hipMemset(t->v, 0, wb);
  if (e == hipSuccess) e = hipMemset(t->count, 0, 2 * sizeof(long long));
  if (e == hipSuccess) e = hipMemset(t->losses, 0, sizeof(double) * (QCE_VAE_TRAINER_SLOTS + 1));
  if (e == hipSuccess) e = hipMemset(t->skipped, 0, sizeof(int) * QCE_VAE_TRAINER_SLOTS);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    release(t);
    return qce_set_error(QCE_EHIP, tr_err(std::string("allocating the trainer failed: ") + hipGetErrorString(e)));
  }
  a.w = t->w;
  a.rows = t->rows;
  a.partials = t->partials;
  a.count = t->count;
  a.count_snap = t->count + 1;
  t->proto = a;
  *out = t;
  return QCE_OK;
}

int qce_vae_trainer_step(qce_vae_trainer* tr, const float* x, int64_t n_x, const float* target, int64_t n_target,
                         const double* snr_db, const int32_t* index, int64_t B, double n_bits, const float* eps,
                         uint64_t seed, uint64_t row_offset, int step_slot, void* stream) {
  QceVaeStepArgs a;
  if (int rc = batch_args("vae_trainer_step", tr, x, n_x, target, n_target, snr_db, index, B, n_bits, eps, seed,
                          row_offset, &a))
    return rc;
  if (step_slot < 0 || step_slot >= QCE_VAE_TRAINER_SLOTS)
    return qce_set_error(QCE_EARG, "vae_trainer_step: step_slot must lie in [0, " + std::to_string(QCE_VAE_TRAINER_SLOTS) + ")");
  DeviceGuard g(tr->device);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(qce_launch_vae_step(a, st));
  QceVaeUpdateArgs u = update_args(tr, B);
  u.w = tr->w;
  u.m = tr->m;
  u.v = tr->v;
  u.loss_out = tr->losses + step_slot;
  u.skipped_out = tr->skipped + step_slot;
  HIPCHK(qce_launch_vae_update(u, st));
  return QCE_OK;
}

int qce_vae_trainer_grads(qce_vae_trainer* tr, const float* x, int64_t n_x, const float* target, int64_t n_target,
                          const double* snr_db, const int32_t* index, int64_t B, double n_bits, const float* eps,
                          uint64_t seed, uint64_t row_offset, float* grads_out, double* rows_out, double* loss_out,
                          void* stream) {
  QceVaeStepArgs a;
  if (int rc = batch_args("vae_trainer_grads", tr, x, n_x, target, n_target, snr_db, index, B, n_bits, eps, seed,
                          row_offset, &a))
    return rc;
  DeviceGuard g(tr->device);
  hipStream_t st = (hipStream_t)stream;
  if (rows_out) a.rows = rows_out;
  HIPCHK(qce_launch_vae_step(a, st));
  QceVaeUpdateArgs u = update_args(tr, B);
  u.rows = a.rows;
  u.loss_out = loss_out ? loss_out : tr->losses + QCE_VAE_TRAINER_SLOTS;
  u.grads_out = grads_out;
  HIPCHK(qce_launch_vae_update(u, st));
  return QCE_OK;
}

int qce_vae_trainer_read(qce_vae_trainer* tr, double* losses_out, int32_t* skipped_out, int n, void* stream) {
  if (!tr) return qce_set_error(QCE_EARG, "vae_trainer_read: null handle");
  if (n < 0 || n > QCE_VAE_TRAINER_SLOTS || (n > 0 && (!losses_out || !skipped_out)))
    return qce_set_error(QCE_EARG, "vae_trainer_read: bad arguments");
  if (n == 0) return QCE_OK;
  DeviceGuard g(tr->device);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(losses_out, tr->losses, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(skipped_out, tr->skipped, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_vae_trainer_get_state(qce_vae_trainer* tr, float* weights_out, float* exp_avg_out, float* exp_avg_sq_out,
                              int64_t* step_out, void* stream) {
  if (!tr) return qce_set_error(QCE_EARG, "vae_trainer_get_state: null handle");
  DeviceGuard g(tr->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t wb = sizeof(float) * (size_t)tr->n_params;
  if (weights_out) HIPCHK(hipMemcpyAsync(weights_out, tr->w, wb, hipMemcpyDeviceToDevice, st));
  if (exp_avg_out) HIPCHK(hipMemcpyAsync(exp_avg_out, tr->m, wb, hipMemcpyDeviceToDevice, st));
  if (exp_avg_sq_out) HIPCHK(hipMemcpyAsync(exp_avg_sq_out, tr->v, wb, hipMemcpyDeviceToDevice, st));
  long long count = 0;
  if (step_out) HIPCHK(hipMemcpyAsync(&count, tr->count, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (step_out) *step_out = count;
  return QCE_OK;
}

int qce_vae_trainer_set_state(qce_vae_trainer* tr, const float* weights, const float* exp_avg, const float* exp_avg_sq,
                              int64_t step, void* stream) {
  if (!tr) return qce_set_error(QCE_EARG, "vae_trainer_set_state: null handle");
  if (step < 0) return qce_set_error(QCE_EARG, "vae_trainer_set_state: the step count cannot be negative");
  DeviceGuard g(tr->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t wb = sizeof(float) * (size_t)tr->n_params;
  if (weights) HIPCHK(hipMemcpyAsync(tr->w, weights, wb, hipMemcpyDeviceToDevice, st));
  if (exp_avg) HIPCHK(hipMemcpyAsync(tr->m, exp_avg, wb, hipMemcpyDeviceToDevice, st));
  if (exp_avg_sq) HIPCHK(hipMemcpyAsync(tr->v, exp_avg_sq, wb, hipMemcpyDeviceToDevice, st));
  const long long count = step;
  HIPCHK(hipMemcpyAsync(tr->count, &count, sizeof(long long), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return QCE_OK;
}

int qce_vae_trainer_destroy(qce_vae_trainer* tr) {
  if (!tr) return QCE_OK;
  DeviceGuard g(tr->device);
  (void)hipDeviceSynchronize();  // steps still in flight use the buffers
  release(tr);
  return QCE_OK;
}

}  // extern "C"
