// C ABI of libqce.so, the training side of the VAE estimator (qce_vae_train.hip): device pointers only,
// asynchronous on the caller's stream, no status to read.  Every refusal happens before a launch.
#include <math.h>

#include <string>

#include "qce_capi.h"
#include "qce_common.h"

namespace {

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int latent_shape(const char* who, int64_t B, int L) {
  if (B < 0 || L < 1) return qce_set_error(QCE_EARG, std::string(who) + ": bad shape");
  if (L > QCE_VAE_MAX_LATENT)
    return qce_set_error(QCE_ENOTIMPL, std::string(who) + ": latent_dim up to " + std::to_string(QCE_VAE_MAX_LATENT) +
                                           ", got " + std::to_string(L));
  return QCE_OK;
}

}  // namespace

extern "C" {

int qce_vae_sample(const float* enc, int64_t B, int L, const float* eps_in, uint64_t seed, uint64_t row_offset,
                   float* z_out, float* eps_out, int device, void* stream) {
  if (int rc = latent_shape("vae_sample", B, L)) return rc;
  if (B > 0 && (!enc || !z_out || (!eps_in && !eps_out))) return qce_set_error(QCE_EARG, "vae_sample: null buffer");
  if (B == 0) return QCE_OK;
  DeviceGuard g(device);
  HIPCHK(qce_launch_vae_sample(enc, eps_in, B, L, seed, row_offset, z_out, eps_out, (hipStream_t)stream));
  return QCE_OK;
}

int qce_vae_sample_bwd(const float* enc, const float* eps, const float* grad_z, int64_t B, int L, float* grad_enc,
                       int device, void* stream) {
  if (int rc = latent_shape("vae_sample_bwd", B, L)) return rc;
  if (B > 0 && (!enc || !eps || !grad_z || !grad_enc)) return qce_set_error(QCE_EARG, "vae_sample_bwd: null buffer");
  if (B == 0) return QCE_OK;
  DeviceGuard g(device);
  HIPCHK(qce_launch_vae_sample_bwd(enc, eps, grad_z, B, L, grad_enc, (hipStream_t)stream));
  return QCE_OK;
}

int qce_vae_elbo(const float* enc, const float* dec, const float* target, int64_t n_target, int64_t B, int N, int L,
                 int mode, double n_bits, const int32_t* index, const double* snr_db, double* rows_out,
                 float* grad_enc, float* grad_dec, int device, void* stream) {
  if (B < 0 || N < 1 || L < 1 || n_target < 0) return qce_set_error(QCE_EARG, "vae_elbo: bad shape");
  if (mode != 0 && mode != 1) return qce_set_error(QCE_EARG, "vae_elbo: mode must be 0 (genie / noisy) or 1 (real)");
  if (!qce_vae_train_shape(N, L))
    return qce_set_error(QCE_ENOTIMPL, "vae_elbo: n_antennas must be a power of two in [16, 256] and latent_dim in [1, " +
                                           std::to_string(QCE_VAE_MAX_LATENT) + "], got " + std::to_string(N) + ", " +
                                           std::to_string(L));
  QceVaeElboArgs a{};
  a.mode = mode;
  if (mode == 1) {
    if (isinf(n_bits) && n_bits > 0) a.n_bits = 0;
    else {
      a.n_bits = (int)n_bits;
      if (!(n_bits >= 1.0) || (double)a.n_bits != n_bits)
        return qce_set_error(QCE_EARG, "vae_elbo: n_bits must be an integer >= 1 or inf");
      if (a.n_bits > 8) return qce_set_error(QCE_ENOTIMPL, "vae_elbo: the 'real' loss covers uniform quantisers up to 8 bits");
      a.step = uniform_std_step(a.n_bits);
    }
    if (B > 0 && !snr_db) return qce_set_error(QCE_EARG, "vae_elbo: mode 1 needs snr_db");
  }
  if (B > 0 && (!enc || !dec || !target || !rows_out || !grad_enc || !grad_dec))
    return qce_set_error(QCE_EARG, "vae_elbo: null buffer");
  if (B > 0 && (index ? n_target < 1 : n_target < B))
    return qce_set_error(QCE_EARG, "vae_elbo: target has fewer rows than the batch uses");
  if (misaligned(dec) || misaligned(target) || misaligned(grad_dec))
    return qce_set_error(QCE_EARG, "vae_elbo: dec, target and grad_dec must be 16-byte aligned");
  if (B == 0) return QCE_OK;
  a.B = B;
  a.T = n_target;
  a.N = N;
  a.L = L;
  a.sqrt_pi_f = sqrtf((float)M_PI);  // torch.sqrt(torch.tensor(torch.pi, dtype=torch.float)), uniform_quantizer.py:110
  a.enc = enc;
  a.dec = dec;
  a.t = target;
  a.index = index;
  a.snr = mode == 1 ? snr_db : nullptr;
  a.rows = rows_out;
  a.g_enc = grad_enc;
  a.g_dec = grad_dec;
  DeviceGuard g(device);
  HIPCHK(qce_launch_vae_elbo(a, (hipStream_t)stream));
  return QCE_OK;
}

}  // extern "C"
