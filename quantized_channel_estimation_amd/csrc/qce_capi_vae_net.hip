// C ABI of libqce.so, the fused inference network of the VAE estimator (qce_vae_net.hip): a handle that owns the
// packed weights, and a forward that optionally continues into the Fourier-domain LMMSE (qce_vae.hip) on the same
// stream.  Every refusal of qce_vae_net_create happens before a device call.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qce_capi.h"
#include "qce_common.h"

struct qce_vae_net {
  int N, P, L, n_layers, genie, device;
  QceVaeNetArgs proto;       // everything but B, dft and the batch pointers
  float* d_raw = nullptr;    // the caller's flat weights
  float* d_packed = nullptr;
  float* lv_scratch = nullptr;  // log-variances of one chunk when the caller wants none
  int64_t lv_rows = 0;
  int* d_status = nullptr;
};

namespace {

constexpr int64_t CHUNK = 1 << 16;  // samples per launch, as qce_vae_estimate

int up(int v, int m) { return (v + m - 1) / m * m; }

std::string net_err(const std::string& msg) { return "vae_net_create: " + msg; }

void release(qce_vae_net* n) {
  if (n->d_raw) (void)hipFree(n->d_raw);
  if (n->d_packed) (void)hipFree(n->d_packed);
  if (n->lv_scratch) (void)hipFree(n->lv_scratch);
  if (n->d_status) (void)hipFree(n->d_status);
  delete n;
}

// One layer (out_keep of its `out` rows) into the lane-major layout of k_vae_net; returns the floats written.
void pack_layer(const float* w, const float* b, int in, int out_keep, QceVaeNetLayer* ly, std::vector<float>* dst) {
  ly->ksteps = up(in, 4) / 4;
  ly->ntiles = up(out_keep, 16) / 16;
  ly->w_off = (int)dst->size();
  dst->resize(dst->size() + (size_t)ly->ntiles * ly->ksteps * 64, 0.0f);
  float* p = dst->data() + ly->w_off;
  for (int nt = 0; nt < ly->ntiles; ++nt)
    for (int ks = 0; ks < ly->ksteps; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int col = nt * 16 + (lane & 15), k = ks * 4 + (lane >> 4);
        if (col < out_keep && k < in) p[((size_t)nt * ly->ksteps + ks) * 64 + lane] = w[(size_t)col * in + k];
      }
  ly->b_off = (int)dst->size();
  dst->resize(dst->size() + (size_t)ly->ntiles * 16, 0.0f);
  for (int c = 0; c < out_keep; ++c) (*dst)[ly->b_off + c] = b[c];
}

}  // namespace

extern "C" {

int qce_vae_net_create(int N, int P, int L, int n_layers, int n_pilot_convs, int genie, const int32_t* widths,
                       const float* weights, int64_t n_weights, int io, int device, qce_vae_net** out) {
  if (!widths || !weights || !out) return qce_set_error(QCE_EARG, net_err("null pointer"));
  *out = nullptr;
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, net_err("bad io"));
  if (P < 1 || n_pilot_convs < 0) return qce_set_error(QCE_EARG, net_err("bad shape"));
  if (N < 16 || N > 256 || (N & (N - 1)))
    return qce_set_error(QCE_ENOTIMPL, net_err("n_antennas must be a power of two in [16, 256], got " + std::to_string(N)));
  if (P > QCE_VAE_MAX_PILOTS)
    return qce_set_error(QCE_ENOTIMPL, net_err("at most " + std::to_string(QCE_VAE_MAX_PILOTS) + " pilots, got " + std::to_string(P)));
  if (L < 1 || L > QCE_VAE_MAX_LATENT)
    return qce_set_error(QCE_ENOTIMPL, net_err("latent_dim must lie in [1, " + std::to_string(QCE_VAE_MAX_LATENT) + "], got " +
                                               std::to_string(L)));
  if (n_layers < 1 || n_layers > QCE_VAE_NET_MAX_LAYERS)
    return qce_set_error(QCE_ENOTIMPL, net_err("n_layers must lie in [1, " + std::to_string(QCE_VAE_NET_MAX_LAYERS) + "], got " +
                                               std::to_string(n_layers)));
  if (n_pilot_convs > QCE_VAE_NET_MAX_CONVS)
    return qce_set_error(QCE_ENOTIMPL, net_err("at most " + std::to_string(QCE_VAE_NET_MAX_CONVS) + " pilot convolutions, got " +
                                               std::to_string(n_pilot_convs)));
  const int32_t* conv = widths;
  const int32_t* enc = conv + n_pilot_convs + 1;
  const int32_t* dec = enc + n_layers + 1;
  const int nw = n_pilot_convs + 1 + 2 * (n_layers + 1);
  for (int i = 0; i < nw; ++i) {
    if (widths[i] < 1) return qce_set_error(QCE_EARG, net_err("widths must be positive"));
    if (widths[i] > QCE_VAE_NET_MAX_WIDTH)
      return qce_set_error(QCE_ENOTIMPL, net_err("layer widths up to " + std::to_string(QCE_VAE_NET_MAX_WIDTH) + ", got " +
                                                 std::to_string(widths[i])));
  }
  if (P > 1 && n_pilot_convs == 0 && !genie)
    return qce_set_error(QCE_EARG, net_err("several pilots need n_pilot_convs >= 1 (the encoder takes one row)"));
  // (without convolutions the list of channel counts is [P] alone: a genie network never uses it)
  if (conv[0] != P || (n_pilot_convs > 0 && conv[n_pilot_convs] != 1) || enc[0] != 2 * N || enc[n_layers] != 2 * L ||
      dec[0] != L || dec[n_layers] != N)
    return qce_set_error(QCE_EARG, net_err("inconsistent widths: conv P .. 1, enc 2N .. 2L, dec L .. N"));
  for (int i = 0; i <= n_pilot_convs; ++i)
    if (conv[i] > QCE_VAE_MAX_PILOTS)
      return qce_set_error(QCE_ENOTIMPL, net_err("pilot convolutions of up to " + std::to_string(QCE_VAE_MAX_PILOTS) + " channels"));
  int64_t implied = 0;
  for (int i = 0; i < n_pilot_convs; ++i) implied += (int64_t)conv[i + 1] * conv[i] + conv[i + 1];
  for (int i = 0; i < n_layers; ++i) implied += (int64_t)enc[i + 1] * enc[i] + enc[i + 1];
  for (int i = 0; i < n_layers; ++i) implied += (int64_t)dec[i + 1] * dec[i] + dec[i + 1];
  if (n_weights != implied)
    return qce_set_error(QCE_EARG, net_err("the widths imply " + std::to_string(implied) + " weights, got " + std::to_string(n_weights)));

  DeviceGuard g(device);
  std::vector<float> raw((size_t)n_weights);
  if (io == QCE_IO_DEVICE) HIPCHK(hipMemcpy(raw.data(), weights, sizeof(float) * raw.size(), hipMemcpyDeviceToHost));
  else memcpy(raw.data(), weights, sizeof(float) * raw.size());

  qce_vae_net* n = new qce_vae_net();
  n->N = N;
  n->P = P;
  n->L = L;
  n->n_layers = n_layers;
  n->genie = genie ? 1 : 0;
  n->device = device;
  QceVaeNetArgs& a = n->proto;
  memset(&a, 0, sizeof(a));
  a.N = N;
  a.P = genie ? 1 : P;
  a.L = L;
  a.nconv = genie ? 0 : n_pilot_convs;
  size_t off = 0;
  for (int i = 0; i < n_pilot_convs; ++i) {
    a.conv_ch[i] = conv[i];
    a.conv_off[i] = (int)off;
    off += (size_t)conv[i + 1] * conv[i] + conv[i + 1];
  }
  a.conv_ch[n_pilot_convs] = conv[n_pilot_convs];
  std::vector<float> packed;
  int widest = 2 * N;
  a.nenc = n_layers;
  a.nlayers = 2 * n_layers;
  for (int half = 0; half < 2; ++half) {
    const int32_t* wd = half ? dec : enc;
    for (int i = 0; i < n_layers; ++i) {
      const int in = wd[i], outw = wd[i + 1];
      const int keep = (!half && i == n_layers - 1) ? L : outw;  // the encoder's last layer: mu only
      QceVaeNetLayer* ly = &a.layer[half * n_layers + i];
      pack_layer(raw.data() + off, raw.data() + off + (size_t)outw * in, in, keep, ly, &packed);
      ly->relu = i < n_layers - 1;
      off += (size_t)outw * in + outw;
      if (16 * ly->ntiles > widest) widest = 16 * ly->ntiles;
      if (4 * ly->ksteps > widest) widest = 4 * ly->ksteps;
    }
  }
  a.stride = up(widest, 64) + 4;  // = 4 mod 64
  a.spp = 1024 / (a.P * N);       // 1024 complex values of FP64 staging, at least one sample
  a.spp = a.spp < 1 ? 1 : (a.spp > QCE_VAE_NET_ROWS ? QCE_VAE_NET_ROWS : a.spp);

  hipError_t e = hipMalloc((void**)&n->d_raw, sizeof(float) * raw.size());
  if (e == hipSuccess) e = hipMalloc((void**)&n->d_packed, sizeof(float) * packed.size());
  if (e == hipSuccess) e = hipMalloc((void**)&n->d_status, sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(n->d_raw, raw.data(), sizeof(float) * raw.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(n->d_packed, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release(n);
    return qce_set_error(QCE_EHIP, net_err(std::string("uploading the weights failed: ") + hipGetErrorString(e)));
  }
  a.raw = n->d_raw;
  a.packed = n->d_packed;
  *out = n;
  return QCE_OK;
}

int qce_vae_net_forward(qce_vae_net* net, const double* net_in, int fft_pre, int64_t B, float* mu_out, float* logvar_out,
                        const double* y, const double* x_cplx, double snr_db, double n_bits, double* h_out, int io,
                        void* stream) {
  if (!net) return qce_set_error(QCE_EARG, "vae_net_forward: null handle");
  if (B < 0) return qce_set_error(QCE_EARG, "vae_net_forward: bad shape");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "vae_net_forward: bad io");
  if (B > 0 && !net_in) return qce_set_error(QCE_EARG, "vae_net_forward: null buffer");
  if (h_out && (!y || !x_cplx)) return qce_set_error(QCE_EARG, "vae_net_forward: an estimate needs y and the pilot vector");
  const int N = net->N, P = net->P, L = net->L;
  QceVaeArgs va;
  if (h_out)
    if (int rc = vae_lmmse_args("vae_net_forward", N, P, x_cplx, snr_db, n_bits, &va)) return rc;
  if (B == 0) return QCE_OK;
  DeviceGuard g(net->device);
  hipStream_t st = (hipStream_t)stream;
  QceVaeNetArgs a = net->proto;
  a.dft = (net->genie || fft_pre) ? 1 : 0;
  const size_t in_row = (size_t)a.P * N;  // complex values per row of net_in
  const int64_t cmax = B < CHUNK ? B : CHUNK;
  const bool host = io == QCE_IO_HOST;
  const bool own_lv = host || !logvar_out;
  if (own_lv && net->lv_rows < cmax) {
    if (net->lv_scratch) HIPCHK(hipFree(net->lv_scratch));  // (waits for the work that still uses it)
    net->lv_scratch = nullptr;
    net->lv_rows = 0;
    HIPCHK(hipMalloc((void**)&net->lv_scratch, sizeof(float) * (size_t)cmax * N));
    net->lv_rows = cmax;
  }
  int status = 0;
  {
    StreamScratch sc(st);
    void *din = nullptr, *dmu = nullptr, *dy = nullptr, *dh = nullptr;
    const bool y_is_in = (const void*)y == (const void*)net_in;
    if (host) {
      HIPCHK(sc.get(&din, sizeof(double2) * (size_t)cmax * in_row));
      if (mu_out) HIPCHK(sc.get(&dmu, sizeof(float) * (size_t)cmax * L));
      if (h_out) {
        if (!y_is_in) HIPCHK(sc.get(&dy, sizeof(double2) * (size_t)cmax * P * N));
        HIPCHK(sc.get(&dh, sizeof(double2) * (size_t)cmax * N));
      }
    }
    if (h_out) {
      HIPCHK(hipMemsetAsync(net->d_status, 0, sizeof(int), st));
      va.status = net->d_status;
      va.lv_f32 = 1;
    }
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
      const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
      const double* in_c = net_in + 2 * (size_t)b0 * in_row;
      a.B = nb;
      if (host) {
        HIPCHK(hipMemcpyAsync(din, in_c, sizeof(double2) * (size_t)nb * in_row, hipMemcpyHostToDevice, st));
        a.in = (const double2*)din;
        a.mu = (float*)dmu;
      } else {
        a.in = (const double2*)in_c;
        a.mu = mu_out ? mu_out + (size_t)b0 * L : nullptr;
      }
      a.lv = own_lv ? net->lv_scratch : logvar_out + (size_t)b0 * N;
      HIPCHK(qce_launch_vae_net(a, st));
      if (host) {
        if (mu_out) HIPCHK(hipMemcpyAsync(mu_out + (size_t)b0 * L, dmu, sizeof(float) * (size_t)nb * L, hipMemcpyDeviceToHost, st));
        if (logvar_out)
          HIPCHK(hipMemcpyAsync(logvar_out + (size_t)b0 * N, a.lv, sizeof(float) * (size_t)nb * N, hipMemcpyDeviceToHost, st));
      }
      if (h_out) {
        const double* y_c = y + 2 * (size_t)b0 * P * N;
        double* h_c = h_out + 2 * (size_t)b0 * N;
        va.B = nb;
        va.lv = a.lv;
        if (host) {
          if (!y_is_in) HIPCHK(hipMemcpyAsync(dy, y_c, sizeof(double2) * (size_t)nb * P * N, hipMemcpyHostToDevice, st));
          va.y = (const double2*)(y_is_in ? din : dy);
          va.h = (double2*)dh;
        } else {
          va.y = (const double2*)y_c;
          va.h = (double2*)h_c;
        }
        HIPCHK(qce_launch_vae(va, st));
        if (host) HIPCHK(hipMemcpyAsync(h_c, dh, sizeof(double2) * (size_t)nb * N, hipMemcpyDeviceToHost, st));
      }
    }
    if (h_out) HIPCHK(hipMemcpyAsync(&status, net->d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_out || host) HIPCHK(hipStreamSynchronize(st));
  }
  if (status)
    return qce_set_error(QCE_ECHOL, "vae_net_forward: the quantised-observation covariance Cr is not positive definite in "
                                    "some DFT bin (the reference's pinv has no counterpart here)");
  return QCE_OK;
}

int qce_vae_net_destroy(qce_vae_net* net) {
  if (!net) return QCE_OK;
  DeviceGuard g(net->device);
  release(net);
  return QCE_OK;
}

}  // extern "C"
