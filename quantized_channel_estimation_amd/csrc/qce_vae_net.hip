// The VAE estimator's inference network in one kernel (reference estimators/vae.py:161-172, the input preparation of
// eval, and :294-309 DNN_VAE.forward_nosamp): observations y (B, P N) complex128 (or the true channels h (B, N) of a
// 'genie' network) in, the decoder's log-variances lv (B, N) float32 out, optionally the latent mean mu (B, L).
// Nothing between the two reaches memory.
//
// k_vae_net: one workgroup (256 threads, four waves) per tile of 16 rows, the M of v_mfma_f32_16x16x4_f32.
//   1. Features.  spp samples at a time, the P rows of N complex values of each go to LDS (row stride N + 1) and
//      through r_fft_rows, the FP64 transform of the feature pass of qce_observe_rows.hip; [Re | Im] times 1 / sqrt(N)
//      is rounded to float32 once, as there.  Without the transform the values themselves are rounded.
//   2. Pilot convolutions (kernel size 1): the whole chain of channel mixes + ReLU is applied to the P feature values of
//      one position in registers; the single channel left, 2N floats per row, is all that reaches the activations.
//   3. Encoder and 4. decoder: every linear layer is X (16 x in) W^T (in x out) on the f32 MFMA.  Lane l holds
//      A[row l & 15][k = l >> 4] from the activation buffer and B[k = l >> 4][col l & 15] from the packed weights (one
//      coalesced dword per lane and k-step: the 64 values of a (column tile, k-step) are contiguous); D is
//      row = 4 (l >> 4) + r, col = l & 15.  A wave owns column tiles wave, wave + 4, ...; for each it runs two
//      accumulators, the even and the odd k-steps (the instruction's dependent latency, 40 cycles, is longer than its
//      issue interval, 32), each a k-ordered fmaf chain: the first starts from the bias, the two are added at the end.
//      Activations ping-pong between two LDS buffers of 16 x stride floats, stride = 4 mod 64 so that the 16 rows x 4 k of
//      an A read, and the 16 x 16 of a D write, fall on 64 different banks.  The second buffer shares its bytes with the
//      transform's staging, which is dead by then.
//      The packed weights are zero beyond (out, in): padded output columns are exactly 0 (0 bias, ReLU(0) = 0) and are
//      the next layer's padded inputs.  The last encoder layer keeps its first L outputs (mu): inference needs no
//      encoder variance.
// Rows past B compute on zeros and store nothing; a row's arithmetic does not depend on its place in the tile or the
// batch (the transform works row by row, an MFMA row sees only its own A values).  No atomics.
//
// Roofline: the packed weights (n256p2: 1.3 MB) are read once per workgroup from L2, 64 FLOP per dword; with
// 64 FLOP / clk / SIMD of the f32 MFMA that is one dword per lane per 32 cycles and wave, far below what L2 delivers, so
// the MFMA issue rate bounds the layers and the launch latency bounds the small networks ("VAE evaluation").
#include "qce_common.h"
#include "qce_kernels.h"
#include "qce_observe_dev.h"

namespace {

constexpr int NET_THREADS = 256;
constexpr int ROWS = QCE_VAE_NET_ROWS;
constexpr int MAXC = QCE_VAE_NET_MAX_CONVS;

QCE_DEV float relu(float v) { return v < 0.0f ? 0.0f : v; }  // keeps a NaN, as torch's does

unsigned up16(size_t v) { return (unsigned)((v + 15) & ~(size_t)15); }

// LDS carve (bytes): activation buffer 0 | activation buffer 1, shared with { staging T | twiddles }
struct NetLds {
  unsigned off_b1, off_tw, bytes;
};
NetLds net_lds(const QceVaeNetArgs& a) {
  NetLds l;
  const unsigned buf = up16(sizeof(float) * (size_t)ROWS * a.stride);
  const unsigned stage = up16(sizeof(double2) * (size_t)a.spp * a.P * (a.N + 1));
  const unsigned tw = up16(sizeof(double2) * (size_t)(a.N / 2));
  l.off_b1 = buf;
  l.off_tw = buf + stage;
  const unsigned second = stage + tw > buf ? stage + tw : buf;
  l.bytes = buf + second;
  return l;
}

__global__ __launch_bounds__(NET_THREADS) void k_vae_net(QceVaeNetArgs a, NetLds lds) {
  extern __shared__ __attribute__((aligned(16))) char n_smem[];
  float* buf0 = reinterpret_cast<float*>(n_smem);
  float* buf1 = reinterpret_cast<float*>(n_smem + lds.off_b1);
  double2* T = reinterpret_cast<double2*>(n_smem + lds.off_b1);
  double2* tw = reinterpret_cast<double2*>(n_smem + lds.off_tw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, P = a.P, RS = N + 1, S = a.stride;
  const int lgN = 31 - __clz(N);
  const long long b0 = (long long)blockIdx.x * ROWS;

  // ---- 1 + 2: features and the pilot convolutions, spp samples per pass -----------------------------------------
  if (a.dft)
    for (int t = tid; t < (N >> 1); t += NET_THREADS) {
      double s, c;
      sincospi(-2.0 * (double)t / (double)N, &s, &c);
      tw[t] = make_double2(c, s);
    }
  const double rs = a.dft ? 1.0 / sqrt((double)N) : 1.0;
  const int PN = P * N;
  for (int s0 = 0; s0 < ROWS; s0 += a.spp) {
    const int ns = ROWS - s0 < a.spp ? ROWS - s0 : a.spp;
    for (int e = tid; e < ns * PN; e += NET_THREADS) {
      const int s = e / PN, r = e - s * PN;
      const long long b = b0 + s0 + s;
      T[(s * P + (r >> lgN)) * RS + (r & (N - 1))] = b < a.B ? a.in[(size_t)b * PN + r] : make_double2(0.0, 0.0);
    }
    __syncthreads();  // (also orders the twiddles before their first use)
    if (a.dft) qce_obs::r_fft_rows<NET_THREADS>(T, ns * P, N, lgN, tw);
    for (int e = tid; e < ns * 2 * N; e += NET_THREADS) {
      const int s = e >> (lgN + 1), q = e & (2 * N - 1), j = q & (N - 1);
      float v[MAXC];
#pragma unroll
      for (int p = 0; p < MAXC; ++p) {
        v[p] = 0.0f;
        if (p < P) {
          const double2 t = T[(s * P + p) * RS + j];
          v[p] = (float)((q < N ? t.x : t.y) * rs);
        }
      }
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        if (i < a.nconv) {
          const int ci = a.conv_ch[i], co = a.conv_ch[i + 1];
          const float* w = a.raw + a.conv_off[i];
          float u[MAXC];
#pragma unroll
          for (int o = 0; o < MAXC; ++o) {
            u[o] = 0.0f;
            if (o < co) {
              float acc = w[co * ci + o];
#pragma unroll
              for (int c = 0; c < MAXC; ++c)
                if (c < ci) acc = fmaf(w[o * ci + c], v[c], acc);
              u[o] = relu(acc);
            }
          }
#pragma unroll
          for (int o = 0; o < MAXC; ++o) v[o] = u[o];
        }
      }
      buf0[(s0 + s) * S + q] = v[0];
    }
    __syncthreads();  // the next pass rewrites T; after the last one buf1 takes its place
  }

  // ---- 3 + 4: the linear layers on the f32 MFMA ----------------------------------------------------------------------
  const int arow = lane & 15, ak = lane >> 4;
  for (int li = 0; li < a.nlayers; ++li) {
    const QceVaeNetLayer ly = a.layer[li];
    const float* src = (li & 1) ? buf1 : buf0;
    float* dst = (li & 1) ? buf0 : buf1;
    const bool last = li == a.nlayers - 1, is_mu = li == a.nenc - 1;
    const float* ap = src + arow * S + ak;
    for (int nt = wave; nt < ly.ntiles; nt += NET_THREADS / 64) {
      const float* wp = a.packed + ly.w_off + (size_t)nt * ly.ksteps * 64 + lane;
      const float bias = a.packed[ly.b_off + nt * 16 + arow];
      f32x4 acc0 = {bias, bias, bias, bias}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
      int ks = 0;
#pragma unroll 4
      for (; ks + 1 < ly.ksteps; ks += 2) {
        acc0 = mfma16x16x4(ap[ks * 4], wp[ks * 64], acc0);
        acc1 = mfma16x16x4(ap[ks * 4 + 4], wp[ks * 64 + 64], acc1);
      }
      if (ks < ly.ksteps) acc0 = mfma16x16x4(ap[ks * 4], wp[ks * 64], acc0);
      const int col = nt * 16 + arow;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * ak + r;
        float v = acc0[r] + acc1[r];
        if (ly.relu) v = relu(v);
        if (!last) dst[row * S + col] = v;
        const long long b = b0 + row;
        if (b < a.B) {
          if (last && col < N) a.lv[(size_t)b * N + col] = v;
          if (is_mu && a.mu && col < a.L) a.mu[(size_t)b * a.L + col] = v;
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

size_t qce_vae_net_lds(const QceVaeNetArgs& a) { return net_lds(a).bytes; }

hipError_t qce_launch_vae_net(const QceVaeNetArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const NetLds l = net_lds(a);
  if (l.bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_vae_net, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes);
    if (e != hipSuccess) return e;
  }
  const long long grid = (a.B + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(k_vae_net, dim3((unsigned)grid), dim3(NET_THREADS), l.bytes, st, a, l);
  return hipGetLastError();
}
