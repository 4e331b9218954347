// Lloyd's k-means for the EM initialisation (sklearn's _kmeans_single_lloyd on dense data with unit weights), FP64 on
// gfx950.  One iteration is
//   k_km_cnorm     |c_k|^2 of the current centres,
//   k_km_assign    scores s_bk = |c_k|^2 - 2 x_b . c_k on the FP64 MFMA, 16 rows x 16 clusters per tile, running minimum
//                  over the cluster blocks (strict <: ties go to the lowest index), labels and per-workgroup counts of
//                  changed labels,
//   k_km_accum     per-chunk cluster sums one-hot(16 clusters x 4 rows) . X(4 rows x 16 columns) on the same MFMA,
//   k_km_sums      the chunk partials added in a fixed order (no floating-point atomics anywhere),
//   k_km_finalize  centres = sums / counts, the squared centre shift, changed labels, empty clusters.
// Distances do not depend on the column order, so X is read in its stored interleaved order (re0, im0, re1, ...), and
// within a group of 16 columns the MFMA's k index runs over the columns in the order that lets a lane fetch its four
// operands with one 32-byte load (both operands use the same order, so the dot products are complete).
#include "qce_common.h"
#include "qce_kmeans.h"

namespace {

constexpr int KM_TPW = 4;  // column tiles (of 16) per accumulation wave

// Fixed-order sum of one value per thread over a workgroup of NT threads (NT a power of two); result on thread 0.
template <int NT>
QCE_DEV double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// one wave per cluster
__global__ __launch_bounds__(256) void k_km_cnorm(int K, int KP, int DP, const double* __restrict__ C,
                                                  double* __restrict__ cnorm) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= KP) return;
  double s = 0.0;
  for (int c = lane; c < DP; c += 64) {
    const double v = C[(size_t)k * DP + c];
    s = fma(v, v, s);
  }
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) cnorm[k] = k < K ? s : __builtin_inf();
}

// A workgroup of W waves takes 16 W rows as W tiles of 16.  The centred tiles sit in LDS in fragment order: the four
// doubles lane l feeds to the four MFMAs of column group g (row l & 15, columns 16 g + 4 (l >> 4) + 0..3) are contiguous
// at ((64 g + l) * 4).  SPLITK (at least W cluster blocks): wave w scores the cluster blocks w, w + W, ... against all W
// tiles, so a centre fragment fetched from L2 feeds W MFMAs; otherwise wave w scores every block against tile w.  The
// waves' minima meet in LDS, where one thread per row combines them (equal scores: the lower cluster index).
template <int W, bool SPLITK>
__global__ __launch_bounds__(64 * W) void k_km_assign(long long B, int D, int DP, int KP, const double* __restrict__ X,
                                                      const double* __restrict__ mean, const double* __restrict__ C,
                                                      const double* __restrict__ cnorm, long long* __restrict__ labels,
                                                      int* __restrict__ pchanged) {
  constexpr int TW = SPLITK ? W : 1;  // tiles per wave
  extern __shared__ __attribute__((aligned(32))) char km_smem[];
  __shared__ double s_best[W][16 * W];
  __shared__ int s_bk[W][16 * W];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* xt = reinterpret_cast<double*>(km_smem);
  const long long r0 = (long long)blockIdx.x * W * 16;
  {
    double* xw = xt + (size_t)wave * 16 * DP;
    for (int c = lane; c < DP; c += 64) {  // the 16 rows' loads of a column go out together
      const double mc = mean[c];
      double v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long row = r0 + wave * 16 + r;
        v[r] = (row < B && c < D) ? X[row * D + c] : mc;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) xw[(((c >> 4) * 64 + ((c >> 2) & 3) * 16 + r) << 2) + (c & 3)] = v[r] - mc;
    }
  }
  for (int e = threadIdx.x; e < W * 16 * W; e += 64 * W) {
    (&s_best[0][0])[e] = __builtin_inf();
    (&s_bk[0][0])[e] = 0;
  }
  __syncthreads();
  const int j = lane & 15, q = lane >> 4;
  const int G = DP >> 4;
  const int t0 = SPLITK ? 0 : wave;
  double best[TW][4];
  int bk[TW][4];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[t][r] = __builtin_inf();
      bk[t][r] = 0;
    }
  }
  const double* xp = xt + (size_t)t0 * 16 * DP + lane * 4;
  for (int kb = SPLITK ? wave * 16 : 0; kb < KP; kb += SPLITK ? 16 * W : 16) {
    const double* cp = C + (size_t)(kb + j) * DP + 4 * q;
    f64x4 acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int g = 0; g < G; ++g) {
      const double4 cv = *reinterpret_cast<const double4*>(cp + g * 16);
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const double4 xv = *reinterpret_cast<const double4*>(xp + (size_t)t * 16 * DP + g * 256);
        acc[t] = mfma16x16x4d(xv.x, cv.x, acc[t]);
        acc[t] = mfma16x16x4d(xv.y, cv.y, acc[t]);
        acc[t] = mfma16x16x4d(xv.z, cv.z, acc[t]);
        acc[t] = mfma16x16x4d(xv.w, cv.w, acc[t]);
      }
    }
    // f64 C/D map: this lane holds rows q + 4 r of each tile, cluster kb + j
    const double cn = cnorm[kb + j];
#pragma unroll
    for (int t = 0; t < TW; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s = fma(-2.0, acc[t][r], cn);
        if (s < best[t][r]) {
          best[t][r] = s;
          bk[t][r] = kb + j;
        }
      }
    }
  }
  // minimum over the 16 lanes of a row group; equal scores keep the lower cluster index
#pragma unroll
  for (int t = 0; t < TW; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const double so = __shfl_xor(best[t][r], m);
        const int ko = __shfl_xor(bk[t][r], m);
        if (so < best[t][r] || (so == best[t][r] && ko < bk[t][r])) {
          best[t][r] = so;
          bk[t][r] = ko;
        }
      }
      if (j == 0) {
        s_best[wave][(t0 + t) * 16 + q + 4 * r] = best[t][r];
        s_bk[wave][(t0 + t) * 16 + q + 4 * r] = bk[t][r];
      }
    }
  }
  __syncthreads();
  if (wave == 0) {  // 16 W <= 64 rows: one thread each
    int changed = 0;
    const long long row = r0 + lane;
    if (lane < 16 * W && row < B) {
      double sb = s_best[0][lane];
      int kbest = s_bk[0][lane];
#pragma unroll
      for (int w = 1; w < W; ++w) {
        const double so = s_best[w][lane];
        const int ko = s_bk[w][lane];
        if (so < sb || (so == sb && ko < kbest)) {
          sb = so;
          kbest = ko;
        }
      }
      changed = labels[row] != (long long)kbest;
      labels[row] = kbest;
    }
    for (int m = 32; m > 0; m >>= 1) changed += __shfl_xor(changed, m);
    if (lane == 0) pchanged[blockIdx.x] = changed;
  }
}

// One wave per (cluster block of 16, KM_TPW column tiles, chunk of rows): A = one-hot(cluster kb + i, row s + q),
// B = x(row s + q, column j); a step whose four rows hold no label of the block is skipped (wave-uniform).
__global__ __launch_bounds__(256) void k_km_accum(long long B, int D, int DP, int KP, long long chunk, int nct,
                                                  const double* __restrict__ X, const double* __restrict__ mean,
                                                  const long long* __restrict__ labels, double* __restrict__ part,
                                                  double* __restrict__ pcount) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int job = blockIdx.x * 4 + wave;
  if (job >= (KP >> 4) * nct) return;
  const int kb = (job / nct) * 16, ct = job % nct;
  const long long s0 = (long long)blockIdx.y * chunk;
  const long long s1 = s0 + chunk < B ? s0 + chunk : B;
  const int i = lane & 15, q = lane >> 4;
  f64x4 acc[KM_TPW];
  int col[KM_TPW];
  double mv[KM_TPW];
#pragma unroll
  for (int t = 0; t < KM_TPW; ++t) {
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    col[t] = (ct * KM_TPW + t) * 16 + i;
    mv[t] = col[t] < D ? mean[col[t]] : 0.0;
  }
  double cnt = 0.0;
  // 16 rows per turn as four MFMA steps of 4: the labels of all four steps are fetched first, then the X values of
  // the steps that hit this cluster block, then the products -- two load latencies per 16 rows
  // (the next turn's labels are fetched a turn ahead; the mean is subtracted only where the products are formed, so no
  // load is waited for before all of a turn's loads are out)
  long long lab[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) lab[u] = s0 + 4 * u + q < s1 ? labels[s0 + 4 * u + q] : -1;
  for (long long s = s0; s < s1; s += 16) {
    double a[4], x[4][KM_TPW];
    bool hit[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = lab[u] == (long long)(kb + i) ? 1.0 : 0.0;
      const long long nrow = s + 16 + 4 * u + q;
      lab[u] = nrow < s1 ? labels[nrow] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long row = s + 4 * u + q;
      hit[u] = __ballot(a[u] != 0.0) != 0ull;  // wave-uniform
      if (hit[u]) {
#pragma unroll
        for (int t = 0; t < KM_TPW; ++t) x[u][t] = (row < s1 && col[t] < D) ? X[row * D + col[t]] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (hit[u]) {
        cnt += a[u];
        // rows past the chunk have a = 0 and pad columns have x = mv = 0: their products are zero
#pragma unroll
        for (int t = 0; t < KM_TPW; ++t) acc[t] = mfma16x16x4d(a[u], x[u][t] - mv[t], acc[t]);
      }
    }
  }
  double* pw = part + (size_t)blockIdx.y * KP * DP;
#pragma unroll
  for (int t = 0; t < KM_TPW; ++t) {
    const int c = (ct * KM_TPW + t) * 16 + i;
    if (c < DP) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[(size_t)(kb + q + 4 * r) * DP + c] = acc[t][r];
    }
  }
  cnt += __shfl_xor(cnt, 16);
  cnt += __shfl_xor(cnt, 32);
  if (ct == 0 && q == 0) pcount[(size_t)blockIdx.y * KP + kb + i] = cnt;
}

// 32 elements per workgroup, 8 threads per element: thread slice j adds the chunks j, j + 8, ... in ascending order, then
// the eight slice sums are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) -- a fixed order
__global__ __launch_bounds__(256) void k_km_sums(int C, int KP, int DP, const double* __restrict__ part,
                                                 const double* __restrict__ pcount, double* __restrict__ sums,
                                                 double* __restrict__ counts) {
  __shared__ double sh[2][8][32];
  const int n = KP * DP;
  const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el;  // n is a multiple of 256: e < n
  double s = 0.0, t = 0.0;
  for (int c = sl; c < C; c += 8) s += part[(size_t)c * n + e];
  if (e < KP)
    for (int c = sl; c < C; c += 8) t += pcount[(size_t)c * KP + e];
  sh[0][sl][el] = s;
  sh[1][sl][el] = t;
  __syncthreads();
  if (sl < 2 && (sl == 0 || e < KP)) {
    const double(*v)[32] = sh[sl];
    const double r = ((v[0][el] + v[1][el]) + (v[2][el] + v[3][el])) + ((v[4][el] + v[5][el]) + (v[6][el] + v[7][el]));
    if (sl == 0) sums[e] = r;
    else counts[e] = r;
  }
}

// one workgroup: every sum below has a fixed order
__global__ __launch_bounds__(1024) void k_km_finalize(int K, int KP, int DP, int nwg, const double* __restrict__ sums,
                                                      const double* __restrict__ counts,
                                                      const int* __restrict__ pchanged, const double* __restrict__ Ccur,
                                                      double* __restrict__ Cnew, double* __restrict__ status) {
  __shared__ double sh[1024];
  const int n = KP * DP;
  double shift = 0.0;
  for (int e = threadIdx.x; e < n; e += 1024) {
    const int k = e / DP;
    double cn = 0.0;
    if (k < K) {
      const double w = counts[k];
      cn = w > 0.0 ? sums[e] / w : sums[e];
      const double d = cn - Ccur[e];
      shift = fma(d, d, shift);
    }
    Cnew[e] = cn;
  }
  double changed = 0.0, empty = 0.0;
  for (int w = threadIdx.x; w < nwg; w += 1024) changed += (double)pchanged[w];
  for (int k = threadIdx.x; k < K; k += 1024) empty += counts[k] == 0.0 ? 1.0 : 0.0;
  const double a = block_sum<1024>(shift, sh);
  __syncthreads();
  const double b = block_sum<1024>(changed, sh);
  __syncthreads();
  const double c = block_sum<1024>(empty, sh);
  if (threadIdx.x == 0) {
    status[0] = a;
    status[1] = b;
    status[2] = c;
  }
}

__global__ __launch_bounds__(256) void k_km_relocate(long long B, int D, int DP, int K, const double* __restrict__ X,
                                                     const double* __restrict__ mean,
                                                     const long long* __restrict__ labels,
                                                     const long long* __restrict__ far, const int* __restrict__ empt,
                                                     int e, double* __restrict__ sums, double* __restrict__ counts) {
  for (int idx = 0; idx < e; ++idx) {
    const long long row = far[idx];
    const int nw = empt[idx];
    if (row < 0 || row >= B || nw < 0 || nw >= K) continue;  // uniform over the workgroup
    const long long old = labels[row];
    if (old < 0 || old >= K) continue;
    for (int c = threadIdx.x; c < D; c += 256) {
      const double x = X[row * D + c] - mean[c];
      sums[(size_t)old * DP + c] -= x;
      sums[(size_t)nw * DP + c] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      counts[nw] = 1.0;
      counts[old] -= 1.0;
    }
    __syncthreads();
  }
}

// one wave per row
__global__ __launch_bounds__(256) void k_km_rowdist(long long B, int D, int DP, int K, const double* __restrict__ X,
                                                    const double* __restrict__ mean, const double* __restrict__ C,
                                                    const long long* __restrict__ labels, double* __restrict__ dist) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  long long lab = labels[row];
  if (lab < 0 || lab >= K) lab = 0;
  double s = 0.0;
  for (int c = lane; c < D; c += 64) {
    const double d = (X[row * D + c] - mean[c]) - C[(size_t)lab * DP + c];
    s = fma(d, d, s);
  }
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) dist[row] = s;
}

__global__ __launch_bounds__(1024) void k_km_vsum(long long n, const double* __restrict__ v, double* __restrict__ out) {
  __shared__ double sh[1024];
  double s = 0.0;
  for (long long e = threadIdx.x; e < n; e += 1024) s += v[e];
  const double t = block_sum<1024>(s, sh);
  if (threadIdx.x == 0) out[0] = t;
}

__global__ __launch_bounds__(256) void k_km_onehot(long long B, int K, const long long* __restrict__ labels,
                                                   double* __restrict__ resp) {
  const long long n = B * K;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const long long b = e / K;
    resp[e] = labels[b] == e - b * K ? 1.0 : 0.0;
  }
}

template <int W, bool SPLITK>
hipError_t launch_assign(const QceKmPlan& p, const double* X, const double* mean, const double* C, const double* cnorm,
                         long long* labels, int* pchanged, hipStream_t st) {
  const size_t lds = sizeof(double) * 16 * (size_t)p.DP * W;
  hipError_t e = hipFuncSetAttribute((const void*)k_km_assign<W, SPLITK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_km_assign<W, SPLITK>), dim3(p.nwg), dim3(64 * W), lds, st, p.B, p.D, p.DP, p.KP, X, mean, C, cnorm,
                     labels, pchanged);
  return hipGetLastError();
}

}  // namespace

QceKmPlan qce_km_plan(long long B, int N, int K) {
  QceKmPlan p;
  p.B = B;
  p.D = 2 * N;
  p.K = K;
  p.DP = (p.D + 15) / 16 * 16;
  p.KP = (K + 15) / 16 * 16;
  // a tile is 128 DP bytes of LDS: four tiles per workgroup up to 32 KB each, two beyond (128 KB in all at DP = 512)
  p.W = p.DP <= 256 ? 4 : 2;
  p.nwg = (int)((B + 16 * p.W - 1) / (16 * p.W));
  // chunks of at least 256 rows (a wave walks its chunk serially, two load latencies per 16 rows, so short chunks and
  // many waves); the (C, KP, DP) partials stay within 64 MB, at most 512 chunks
  long long cmax = (64ll << 20) / ((long long)p.KP * p.DP * 8);
  cmax = cmax < 8 ? 8 : cmax > 512 ? 512 : cmax;
  long long C = (B + 255) / 256;
  C = C > cmax ? cmax : C;
  p.chunk = ((B + C - 1) / C + 15) / 16 * 16;
  p.C = (int)((B + p.chunk - 1) / p.chunk);
  p.nct = (p.DP / 16 + KM_TPW - 1) / KM_TPW;
  return p;
}

hipError_t qce_launch_km_cnorm(const QceKmPlan& p, const double* C, double* cnorm, hipStream_t st) {
  hipLaunchKernelGGL(k_km_cnorm, dim3(p.KP / 4), dim3(256), 0, st, p.K, p.KP, p.DP, C, cnorm);
  return hipGetLastError();
}

hipError_t qce_launch_km_assign(const QceKmPlan& p, const double* X, const double* mean, const double* C,
                                const double* cnorm, long long* labels, int* pchanged, hipStream_t st) {
  const bool splitk = p.KP / 16 >= p.W;  // a cluster block for every wave
  if (p.W == 4)
    return splitk ? launch_assign<4, true>(p, X, mean, C, cnorm, labels, pchanged, st)
                  : launch_assign<4, false>(p, X, mean, C, cnorm, labels, pchanged, st);
  return splitk ? launch_assign<2, true>(p, X, mean, C, cnorm, labels, pchanged, st)
                : launch_assign<2, false>(p, X, mean, C, cnorm, labels, pchanged, st);
}

hipError_t qce_launch_km_accum(const QceKmPlan& p, const double* X, const double* mean, const long long* labels,
                               double* part, double* pcount, hipStream_t st) {
  const int njobs = (p.KP / 16) * p.nct;
  hipLaunchKernelGGL(k_km_accum, dim3((njobs + 3) / 4, p.C), dim3(256), 0, st, p.B, p.D, p.DP, p.KP, p.chunk, p.nct, X,
                     mean, labels, part, pcount);
  return hipGetLastError();
}

hipError_t qce_launch_km_sums(const QceKmPlan& p, const double* part, const double* pcount, double* sums,
                              double* counts, hipStream_t st) {
  const int g = p.KP * p.DP / 32;
  hipLaunchKernelGGL(k_km_sums, dim3(g), dim3(256), 0, st, p.C, p.KP, p.DP, part, pcount, sums, counts);
  return hipGetLastError();
}

hipError_t qce_launch_km_finalize(const QceKmPlan& p, const double* sums, const double* counts, const int* pchanged,
                                  const double* Ccur, double* Cnew, double* status, hipStream_t st) {
  hipLaunchKernelGGL(k_km_finalize, dim3(1), dim3(1024), 0, st, p.K, p.KP, p.DP, p.nwg, sums, counts, pchanged, Ccur,
                     Cnew, status);
  return hipGetLastError();
}

hipError_t qce_launch_km_relocate(const QceKmPlan& p, const double* X, const double* mean, const long long* labels,
                                  const long long* far, const int* empt, int e, double* sums, double* counts,
                                  hipStream_t st) {
  hipLaunchKernelGGL(k_km_relocate, dim3(1), dim3(256), 0, st, p.B, p.D, p.DP, p.K, X, mean, labels, far, empt, e, sums,
                     counts);
  return hipGetLastError();
}

hipError_t qce_launch_km_rowdist(const QceKmPlan& p, const double* X, const double* mean, const double* C,
                                 const long long* labels, double* dist, hipStream_t st) {
  hipLaunchKernelGGL(k_km_rowdist, dim3((unsigned)((p.B + 3) / 4)), dim3(256), 0, st, p.B, p.D, p.DP, p.K, X, mean, C,
                     labels, dist);
  return hipGetLastError();
}

hipError_t qce_launch_km_vsum(long long n, const double* v, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_km_vsum, dim3(1), dim3(1024), 0, st, n, v, out);
  return hipGetLastError();
}

hipError_t qce_launch_km_onehot(const QceKmPlan& p, const long long* labels, double* resp, hipStream_t st) {
  long long g = (p.B * p.K + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(k_km_onehot, dim3((unsigned)g), dim3(256), 0, st, p.B, p.K, labels, resp);
  return hipGetLastError();
}
