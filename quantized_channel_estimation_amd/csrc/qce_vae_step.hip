// One training step of the VAE estimator in two kernels (reference estimators/vae.py:108-123: forward, vae_loss,
// backward, Adam).
//
// k_vae_step: one workgroup (256 threads, four waves) per tile of 16 batch rows, the M of v_mfma_f32_16x16x4_f32.
//   1. Gather.  Row b of the tile is row index[b] of x (clamped to the array, as k_vae_elbo clamps; without an index,
//      row b); rows past B are zeros.
//   2. Pilot convolutions (kernel size 1) as weighted sums over the channels, the whole chain + ReLU in registers per
//      (row, position); the raw tile stays in LDS and the chain is recomputed in the backward pass.
//   3. Encoder, z = mu + exp(s) eps (FP64, rounded once; eps read, or drawn as k_vae_sample draws it), decoder.  A
//      linear layer is X (16 x in) W^T on the f32 MFMA: lane l holds A[row l & 15][k = l >> 4] from the activations in
//      LDS and B[k][col l & 15] = W[col][k] from the plain (out, in) weights in global memory (L2); D is
//      row = 4 (l >> 4) + r, col = l & 15.  A wave owns column tiles wave, wave + 4, ... and runs the even and the odd
//      k-steps in two accumulators, the first started from the bias (k_vae_net's schedule).  Every layer's input stays
//      in LDS in a buffer of its own, 16 x (width rounded up to 16, + 4) floats, so that the 16 rows x 4 k of an A read
//      fall on 64 different banks; columns past the width are exact zeros (zero weights and bias stand in for them).
//   4. Loss.  The row ELBO and its gradients with respect to the encoder and decoder outputs are elbo_row of
//      qce_vae_row_dev.h, the function k_vae_elbo calls, on the rows in LDS: FP64, 1 / B included, rounded to float32.
//   5. Backward, layer by layer from the decoder's last: dW = delta^T a is (out x 16)(16 x in), four k-steps per
//      16 x 16 tile of dW (A = delta^T, B = a, both from LDS); db = the column sums of delta in row order;
//      delta_prev = (delta W) (.) [a > 0] with W as the B operand in its plain layout (coalesced).  Between decoder and
//      encoder g_mu = g_z + KL part, g_s = (float)(g_z exp(s) eps) + KL part, the arithmetic of k_vae_sample_bwd plus
//      torch's float32 addition.  The convolutions' gradients are accumulated per thread in registers over its
//      (row, position) elements, staged in LDS and summed over the 256 threads in thread order.
//   6. The workgroup writes its partial gradient to partials[tile][n_params].  No atomics, nothing passes between
//      workgroups; rows past B have delta = 0 and contribute exact zeros.
//
// k_vae_update: one thread per parameter sums the tile partials in tile order (float32); every workgroup forms the
// loss -mean_b l_b in FP64 in the same order; the skip rule (NaN or > 1000: nothing but the loss and the flag is
// written); torch's Adam with its defaults, each of m, v and w computed in FP64 from the float32 state and rounded
// once.  The step count is read from a copy k_vae_step made, so the thread that advances it races with nobody.
#include "qce_common.h"
#include "qce_kernels.h"
#include "qce_vae_row_dev.h"

namespace {

using namespace qce_vae_row;

constexpr int ST_THREADS = 256;
constexpr int ROWS = QCE_VAE_NET_ROWS;
constexpr int MAXC = QCE_VAE_NET_MAX_CONVS;
constexpr int MAXP = QCE_VAE_MAX_PILOTS;
constexpr int CONV_SLOTS = MAXP * MAXP + MAXP;  // weight (out, in) and bias accumulators of one convolution

QCE_DEV float relu(float v) { return v < 0.0f ? 0.0f : v; }  // keeps a NaN, as torch's does

// dst (16 x up16(out)) = [relu](src (16 x in) W^T + b)
QCE_DEV void layer_forward(const QceVaeStepLayer& ly, const float* __restrict__ w, float* lds, int lane, int wave) {
  const int arow = lane & 15, ak = lane >> 4;
  const int ksteps = (ly.in + 3) >> 2, ntiles = (ly.out + 15) >> 4;
  const float* ap = lds + ly.src + arow * ly.s_src + ak;
  float* dst = lds + ly.dst;
  for (int nt = wave; nt < ntiles; nt += ST_THREADS / 64) {
    const int col = nt * 16 + arow;
    const bool cok = col < ly.out;
    const float bias = cok ? w[ly.b_off + col] : 0.0f;
    const float* wp = w + ly.w_off + (size_t)(cok ? col : 0) * ly.in;
    f32x4 acc0 = {bias, bias, bias, bias}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    int ks = 0;
    for (; ks + 1 < ksteps; ks += 2) {
      const int k0 = ks * 4 + ak, k1 = k0 + 4;
      acc0 = mfma16x16x4(ap[ks * 4], (cok && k0 < ly.in) ? wp[k0] : 0.0f, acc0);
      acc1 = mfma16x16x4(ap[ks * 4 + 4], (cok && k1 < ly.in) ? wp[k1] : 0.0f, acc1);
    }
    if (ks < ksteps) {
      const int k0 = ks * 4 + ak;
      acc0 = mfma16x16x4(ap[ks * 4], (cok && k0 < ly.in) ? wp[k0] : 0.0f, acc0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc0[r] + acc1[r];
      if (ly.relu) v = relu(v);
      dst[(4 * ak + r) * ly.s_dst + col] = v;
    }
  }
}

// dprev (16 x up16(in)) = d (16 x out) W, times [src > 0] with `mask`
QCE_DEV void layer_backward_delta(const QceVaeStepLayer& ly, const float* __restrict__ w, const float* lds, const float* d,
                                  float* dprev, int sd, bool mask, int lane, int wave) {
  const int arow = lane & 15, ak = lane >> 4;
  const int ksteps = (ly.out + 3) >> 2, ntiles = (ly.in + 15) >> 4;
  const float* ap = d + arow * sd + ak;
  const float* src = lds + ly.src;
  for (int nt = wave; nt < ntiles; nt += ST_THREADS / 64) {
    const int col = nt * 16 + arow;
    const bool cok = col < ly.in;
    const float* wp = w + ly.w_off + (cok ? col : 0);
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    int ks = 0;
    for (; ks + 1 < ksteps; ks += 2) {
      const int k0 = ks * 4 + ak, k1 = k0 + 4;
      acc0 = mfma16x16x4(ap[ks * 4], (cok && k0 < ly.out) ? wp[(size_t)k0 * ly.in] : 0.0f, acc0);
      acc1 = mfma16x16x4(ap[ks * 4 + 4], (cok && k1 < ly.out) ? wp[(size_t)k1 * ly.in] : 0.0f, acc1);
    }
    if (ks < ksteps) {
      const int k0 = ks * 4 + ak;
      acc0 = mfma16x16x4(ap[ks * 4], (cok && k0 < ly.out) ? wp[(size_t)k0 * ly.in] : 0.0f, acc0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * ak + r;
      float v = acc0[r] + acc1[r];
      if (mask && !(src[row * ly.s_src + col] > 0.0f)) v = 0.0f;
      dprev[row * sd + col] = v;
    }
  }
}

// part[w_off ..] = d^T (out x 16) src (16 x in); part[b_off ..] = column sums of d
QCE_DEV void layer_grad(const QceVaeStepLayer& ly, const float* lds, const float* d, int sd, float* __restrict__ part,
                        int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int arow = lane & 15, ak = lane >> 4;
  const int otn = (ly.out + 15) >> 4, itn = (ly.in + 15) >> 4;
  const float* src = lds + ly.src;
  for (int tile = wave; tile < otn * itn; tile += ST_THREADS / 64) {
    const int ot = tile / itn, it = tile - ot * itn;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < ROWS / 4; ++ks) {
      const int b = ks * 4 + ak;
      acc = mfma16x16x4(d[b * sd + ot * 16 + arow], src[b * ly.s_src + it * 16 + arow], acc);
    }
    const int i = it * 16 + arow;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = ot * 16 + 4 * ak + r;
      if (o < ly.out && i < ly.in) part[ly.w_off + (size_t)o * ly.in + i] = acc[r];
    }
  }
  for (int o = tid; o < ly.out; o += ST_THREADS) {
    float s = 0.0f;
#pragma unroll
    for (int b = 0; b < ROWS; ++b) s += d[b * sd + o];
    part[ly.b_off + o] = s;
  }
}

// The chain of pilot convolutions on the channel values vs[0][.] of one (row, position): vs[i + 1][.] = ReLU(W_i vs[i] + b_i)
QCE_DEV void conv_chain(const QceVaeStepArgs& a, float (&vs)[MAXC + 1][MAXP]) {
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    if (i < a.nconv) {
      const int ci = a.conv_ch[i], co = a.conv_ch[i + 1];
      const float* w = a.w + a.conv_off[i];
#pragma unroll
      for (int o = 0; o < MAXP; ++o) {
        float u = 0.0f;
        if (o < co) {
          float acc = w[co * ci + o];
#pragma unroll
          for (int c = 0; c < MAXP; ++c)
            if (c < ci) acc = fmaf(w[o * ci + c], vs[i][c], acc);
          u = relu(acc);
        }
        vs[i + 1][o] = u;
      }
    }
  }
}

template <int G, int E, int MODE>
__global__ __launch_bounds__(ST_THREADS) void k_vae_step(QceVaeStepArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_smem[];
  __shared__ long long s_xrow[ROWS], s_trow[ROWS];
  float* lds = reinterpret_cast<float*>(s_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, L = a.L, W2 = 2 * N, RW = a.P * W2;
  const long long b0 = (long long)blockIdx.x * ROWS;
  if (blockIdx.x == 0 && tid == 0) *a.count_snap = *a.count;

  // ---- 1: gather -------------------------------------------------------------------------------------------------
  if (tid < ROWS) {
    const long long b = b0 + tid < a.B ? b0 + tid : a.B - 1;  // rows past the batch: the last row's target, no x
    long long xr = b, tr = b;
    if (a.index) {
      const int ix = a.index[b];
      xr = ix < 0 ? 0 : (ix >= a.n_x ? a.n_x - 1 : ix);
      tr = ix < 0 ? 0 : (ix >= a.T ? a.T - 1 : ix);
    }
    s_xrow[tid] = xr;
    s_trow[tid] = tr;
  }
  __syncthreads();
  const QceVaeStepLayer l0 = a.layer[0];
  {
    float* xdst = lds + (a.nconv ? a.x_off : l0.src);
    const int xs = a.nconv ? RW : l0.s_src;
    for (int e = tid; e < ROWS * RW; e += ST_THREADS) {
      const int r = e / RW, q = e - r * RW;
      xdst[r * xs + q] = b0 + r < a.B ? a.x[(size_t)s_xrow[r] * RW + q] : 0.0f;
    }
  }
  // ---- 2: pilot convolutions -----------------------------------------------------------------------------------------
  if (a.nconv) {
    __syncthreads();
    const float* xraw = lds + a.x_off;
    for (int e = tid; e < ROWS * W2; e += ST_THREADS) {
      const int r = e / W2, q = e - r * W2;
      float vs[MAXC + 1][MAXP];
#pragma unroll
      for (int p = 0; p < MAXP; ++p) vs[0][p] = p < a.P ? xraw[r * RW + p * W2 + q] : 0.0f;
      conv_chain(a, vs);
      float out = vs[0][0];
#pragma unroll
      for (int i = 0; i < MAXC; ++i)
        if (i < a.nconv) out = vs[i + 1][0];
      lds[l0.src + r * l0.s_src + q] = out;
    }
  }
  __syncthreads();

  // ---- 3: encoder, z, decoder ----------------------------------------------------------------------------------------
  const QceVaeStepLayer lmu = a.layer[a.nenc - 1], lz = a.layer[a.nenc], lout = a.layer[a.nlayers - 1];
  float* epsb = lds + a.eps_off;
  for (int li = 0; li < a.nlayers; ++li) {
    if (li == a.nenc) {
      const int LP = (L + 15) & ~15;
      for (int e = tid; e < ROWS * LP; e += ST_THREADS) {
        const int r = e / LP, l = e - r * LP;
        float z = 0.0f;
        if (l < L) {
          const long long b = b0 + r;
          float ep = 0.0f;
          if (b < a.B)
            ep = a.eps ? a.eps[(size_t)b * L + l]
                       : (float)eps_draw(a.seed, (a.row_offset + (unsigned long long)b) * (unsigned long long)L + (unsigned)l);
          epsb[r * L + l] = ep;
          const float* er = lds + lmu.dst + r * lmu.s_dst;
          z = (float)((double)er[l] + exp((double)er[L + l]) * (double)ep);
        }
        lds[lz.src + r * lz.s_src + l] = z;
      }
      __syncthreads();
    }
    layer_forward(a.layer[li], a.w, lds, lane, wave);
    __syncthreads();
  }

  // ---- 4: the row ELBO and its gradients -----------------------------------------------------------------------------
  const int sd = a.s_delta;
  float* dcur = lds + a.d0_off;
  float* doth = lds + a.d1_off;
  float* kl = lds + a.kl_off;
  {
    constexpr int RPP = ST_THREADS / G;  // rows per pass
    const int j = tid & (G - 1);
    const RealConst rc{a.n_bits, a.step, a.sqrt_pi_f};
    for (int r = tid / G; r < ROWS; r += RPP) {
      const long long b = b0 + r;
      const bool live = b < a.B;
      const float* t = a.t + (size_t)s_trow[r] * W2;
      float* ge = kl + r * 2 * L;
      float* gd = dcur + r * sd;
      const double acc = elbo_row<G, E, MODE>(j, live, L, (double)a.B, lds + lmu.dst + r * lmu.s_dst, ge,
                                              lds + lout.dst + r * lout.s_dst, t, t + N,
                                              MODE == 1 ? a.snr + s_trow[r] : nullptr, rc, gd);
      if (live) {
        if (j == 0) a.rows[b] = acc;
      } else {
        for (int l = j; l < 2 * L; l += G) ge[l] = 0.0f;
#pragma unroll
        for (int k = 0; k < E; ++k) gd[j * E + k] = 0.0f;
      }
    }
  }
  __syncthreads();

  // ---- 5 + 6: backward -----------------------------------------------------------------------------------------------
  float* part = a.partials + (size_t)blockIdx.x * a.n_params;
  for (int li = a.nlayers - 1; li >= 0; --li) {
    if (li == a.nenc - 1) {  // dcur holds g_z: through the reparameterisation, plus the KL part
      const int LP2 = (2 * L + 15) & ~15;
      for (int e = tid; e < ROWS * LP2; e += ST_THREADS) {
        const int r = e / LP2, c = e - r * LP2;
        float v = 0.0f;
        if (c < L) {
          v = dcur[r * sd + c] + kl[r * 2 * L + c];
        } else if (c < 2 * L) {
          const int l = c - L;
          const float s = lds[lmu.dst + r * lmu.s_dst + c];
          v = (float)((double)dcur[r * sd + l] * exp((double)s) * (double)epsb[r * L + l]) + kl[r * 2 * L + c];
        }
        doth[r * sd + c] = v;
      }
      __syncthreads();
      float* t = dcur;
      dcur = doth;
      doth = t;
    }
    const QceVaeStepLayer ly = a.layer[li];
    layer_grad(ly, lds, dcur, sd, part, tid);
    if (li > 0 || a.nconv) {
      // the decoder's first input is z and the encoder's first is x or the convolutions' output: no ReLU mask here
      layer_backward_delta(ly, a.w, lds, dcur, doth, sd, li != a.nenc && li != 0, lane, wave);
      float* t = dcur;
      dcur = doth;
      doth = t;
    }
    __syncthreads();
  }

  if (a.nconv) {  // dcur: the gradient of the convolutions' output (16 x 2N)
    float acc[MAXC][CONV_SLOTS];
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
#pragma unroll
      for (int s = 0; s < CONV_SLOTS; ++s) acc[i][s] = 0.0f;
    const float* xraw = lds + a.x_off;
    for (int e = tid; e < ROWS * W2; e += ST_THREADS) {
      const int r = e / W2, q = e - r * W2;
      float vs[MAXC + 1][MAXP];
#pragma unroll
      for (int p = 0; p < MAXP; ++p) vs[0][p] = p < a.P ? xraw[r * RW + p * W2 + q] : 0.0f;
      conv_chain(a, vs);
      float g[MAXP] = {dcur[r * sd + q], 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = MAXC - 1; i >= 0; --i) {
        if (i < a.nconv) {
          const int ci = a.conv_ch[i], co = a.conv_ch[i + 1];
          const float* w = a.w + a.conv_off[i];
          float gin[MAXP] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int o = 0; o < MAXP; ++o) {
            if (o < co) {
              const float gp = vs[i + 1][o] > 0.0f ? g[o] : 0.0f;
              acc[i][MAXP * MAXP + o] += gp;
#pragma unroll
              for (int c = 0; c < MAXP; ++c) {
                if (c < ci) {
                  acc[i][o * MAXP + c] = fmaf(gp, vs[i][c], acc[i][o * MAXP + c]);
                  gin[c] = fmaf(w[o * ci + c], gp, gin[c]);
                }
              }
            }
          }
#pragma unroll
          for (int c = 0; c < MAXP; ++c) g[c] = gin[c];
        }
      }
    }
    // the activations are dead: their bytes stage the 256 per-thread sums of every convolution parameter
    float* red = lds + a.red_off;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      if (i < a.nconv) {
        const int ci = a.conv_ch[i], co = a.conv_ch[i + 1];
#pragma unroll
        for (int o = 0; o < MAXP; ++o) {
          if (o < co) {
            red[(a.conv_off[i] + co * ci + o) * ST_THREADS + tid] = acc[i][MAXP * MAXP + o];
#pragma unroll
            for (int c = 0; c < MAXP; ++c)
              if (c < ci) red[(a.conv_off[i] + o * ci + c) * ST_THREADS + tid] = acc[i][o * MAXP + c];
          }
        }
      }
    }
    __syncthreads();
    for (int p = tid; p < a.n_conv_params; p += ST_THREADS) {
      float s = 0.0f;
      for (int t = 0; t < ST_THREADS; ++t) s += red[p * ST_THREADS + t];
      part[p] = s;
    }
  } else {
    // a genie network carries the convolutions' parameters without using them: their gradient is zero
    for (int p = tid; p < a.layer[0].w_off; p += ST_THREADS) part[p] = 0.0f;
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_vae_update(QceVaeUpdateArgs a) {
  __shared__ double red[ST_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long b = tid; b < a.B; b += ST_THREADS) s += a.rows[b];
  red[tid] = s;
  __syncthreads();
  for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double loss = -red[0] / (double)a.B;
  const bool skip = !(loss <= QCE_VAE_LOSS_SKIP);  // NaN, or above the bound
  const long long t1 = *a.count_snap + 1;
  if (blockIdx.x == 0 && tid == 0) {
    *a.loss_out = loss;
    if (a.skipped_out) *a.skipped_out = skip ? 1 : 0;
    if (a.w && !skip) *a.count = t1;
  }
  const int i = blockIdx.x * ST_THREADS + tid;
  if (i >= a.n_params) return;
  float g = 0.0f;
  for (int t = 0; t < a.tiles; ++t) g += a.partials[(size_t)t * a.n_params + i];
  if (a.grads_out) a.grads_out[i] = g;
  if (!a.w || skip) return;
  constexpr double B1 = 0.9, B2 = 0.999, EPS = 1e-8;  // torch.optim.Adam's defaults
  const double bc1 = 1.0 - pow(B1, (double)t1), bc2 = 1.0 - pow(B2, (double)t1);
  const double gd = (double)g;
  const float m = (float)(B1 * (double)a.m[i] + (1.0 - B1) * gd);
  const float v = (float)(B2 * (double)a.v[i] + (1.0 - B2) * gd * gd);
  a.m[i] = m;
  a.v[i] = v;
  a.w[i] = (float)((double)a.w[i] - (a.lr / bc1) * (double)m / (sqrt((double)v) / sqrt(bc2) + EPS));
}

template <int G, int E>
hipError_t launch_step(const QceVaeStepArgs& a, dim3 grid, hipStream_t st) {
  const void* fn = a.mode == 0 ? (const void*)k_vae_step<G, E, 0> : (const void*)k_vae_step<G, E, 1>;
  if (a.lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_bytes);
    if (e != hipSuccess) return e;
  }
  if (a.mode == 0) hipLaunchKernelGGL((k_vae_step<G, E, 0>), grid, dim3(ST_THREADS), a.lds_bytes, st, a);
  else hipLaunchKernelGGL((k_vae_step<G, E, 1>), grid, dim3(ST_THREADS), a.lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t qce_launch_vae_step(const QceVaeStepArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipErrorInvalidValue;
  const long long tiles = (a.B + ROWS - 1) / ROWS;
  if (tiles > 0x7fffffffLL || a.n_bits < 0 || a.n_bits > 8) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles);
  switch (a.N) {
    case 16: return launch_step<16, 1>(a, grid, st);
    case 32: return launch_step<32, 1>(a, grid, st);
    case 64: return launch_step<64, 1>(a, grid, st);
    case 128: return launch_step<64, 2>(a, grid, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t qce_launch_vae_update(const QceVaeUpdateArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.n_params <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vae_update, dim3((unsigned)((a.n_params + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0, st, a);
  return hipGetLastError();
}
