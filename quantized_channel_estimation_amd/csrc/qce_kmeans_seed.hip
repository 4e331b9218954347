// k-means++ seeding for the EM initialisation (sklearn's _kmeans_plusplus on dense data with unit weights) from
// uniforms the host drew in advance, FP64 on gfx950.  The state is closest[b], the squared distance of row b to the
// nearest chosen centre, kept as one row of a (T, stride) scratch buffer with per-chunk partial sums.  One step is
//   k_km_seed_pick   (one workgroup) the potentials of the T candidates of the last pass from their chunk partials,
//                    the first minimum (np.argmin) -> the new centre, its potential and its scratch row; then, one wave
//                    per trial, the row whose inclusive cumulative sum of closest first reaches u * pot
//                    (np.searchsorted, side "left"), found level by level without the cumulative sum being stored,
//   k_km_seed_cand   one pass over X: for every row the T squared distances to the candidate rows in the difference
//                    form, the minimum of each with closest[b], written to the other scratch buffer with the partial
//                    sums of every chunk.
// No floating-point atomics; every sum has a fixed order:
//   a distance     16 lanes per row; lane l adds the complex elements l, l + 16, ... in ascending order (re, then im),
//                  then the 16 lane sums meet pairwise over the lane bits TP/2, ..., 1, 8, ..., TP (TP = T rounded up to
//                  a power of two: a reduce-scatter that leaves the distance to candidate t on lane t),
//   a chunk        (a multiple of 32 rows, at most 1024 chunks) row 32 i + 8 w + 2 g + {0, 1} belongs to wave w, lane
//                  group g: each (w, g) adds its rows in ascending order, the four groups of a wave meet as
//                  (g0 + g1) + (g2 + g3), the four waves are added in ascending order,
//   a potential    chunks in groups of 32: every group adds its chunks in ascending order, the groups are added in
//                  ascending order.
// The search walks the same levels: groups, the chunks of a group, the 64 segments of a chunk (each the ascending sum
// of its rows), the rows of a segment -- at every level ascending running sums from the level's exclusive prefix, the
// last entry of a level taking the level's own inclusive value (so an entry is always found).
#include "qce_common.h"
#include "qce_kmeans.h"

namespace {

constexpr int KS_GROUP = 32;  // chunks per group of the potential sum
constexpr int KS_SEGS = 64;   // segments per chunk of the search

constexpr int pow2_at_least(int t) { return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : 16; }

// v[t] (t < TP) holds lane l's part of sum t; on return lane l of every 16 holds the whole sum t = l & (TP - 1).
template <int TP>
QCE_DEV double lane_sums(double (&v)[TP], int l) {
#pragma unroll
  for (int h = TP / 2; h >= 1; h >>= 1) {  // h sums are left after the step
    const bool up = (l & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const double keep = up ? v[h + i] : v[i];
      const double send = up ? v[i] : v[h + i];
      v[i] = keep + __shfl_xor(send, h);
    }
  }
  double s = v[0];
#pragma unroll
  for (int m = 8; m >= TP; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

template <int T>
__global__ __launch_bounds__(256) void k_km_seed_cand(long long B, int N, int NP, long long chunk, long long stride,
                                                       int C, const double2* __restrict__ X,
                                                       const double2* __restrict__ mean,
                                                       const long long* __restrict__ cand,
                                                       const double* __restrict__ closest_base,
                                                       const int* __restrict__ win, double* __restrict__ out,
                                                       double* __restrict__ part) {
  constexpr int TP = pow2_at_least(T);
  extern __shared__ __attribute__((aligned(16))) char ks_smem[];
  __shared__ double s_part[4][16];
  double2* s_mean = reinterpret_cast<double2*>(ks_smem);  // NP, zero beyond N
  double2* s_cand = s_mean + NP;                           // (T, NP) centred candidate rows, zero beyond N
  for (int e = threadIdx.x; e < NP; e += 256) {
    const double2 m = (e < N && mean) ? mean[e] : make_double2(0.0, 0.0);
    s_mean[e] = m;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      long long j = cand[t];
      j = j < 0 ? 0 : j >= B ? B - 1 : j;
      double2 v = make_double2(0.0, 0.0);
      if (e < N) v = csub(X[j * N + e], m);
      s_cand[t * NP + e] = v;
    }
  }
  __syncthreads();
  const double* closest = nullptr;
  if (closest_base) {
    int w = win[0];
    w = w < 0 ? 0 : w > 15 ? 15 : w;
    closest = closest_base + (size_t)w * stride;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, l = lane & 15;
  const long long base = (long long)blockIdx.x * chunk;
  double psum = 0.0;  // lane (g, t = l): the chunk's rows of this wave and group
  for (long long rb = base + wave * 8 + 2 * g; rb < base + chunk; rb += 32) {
    const bool v0 = rb < B, v1 = rb + 1 < B;
    const double2* x0 = X + rb * N;
    const double2* x1 = x0 + N;
    double acc0[TP], acc1[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) acc0[t] = acc1[t] = 0.0;
    for (int e0 = 0; e0 < NP; e0 += 64) {
      double2 a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // the loads of both rows go out together
        const int e = e0 + 16 * u + l;
        a[u] = (v0 && e < N) ? x0[e] : make_double2(0.0, 0.0);
        b[u] = (v1 && e < N) ? x1[e] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 16 * u + l;
        const double2 m = s_mean[e];
        const double2 xa = csub(a[u], m), xb = csub(b[u], m);
#pragma unroll
        for (int t = 0; t < T; ++t) {  // pad elements: x, mean and candidate are all zero
          const double2 c = s_cand[t * NP + e];
          double d = xa.x - c.x;
          acc0[t] = fma(d, d, acc0[t]);
          d = xa.y - c.y;
          acc0[t] = fma(d, d, acc0[t]);
          d = xb.x - c.x;
          acc1[t] = fma(d, d, acc1[t]);
          d = xb.y - c.y;
          acc1[t] = fma(d, d, acc1[t]);
        }
      }
    }
    const double d0 = lane_sums<TP>(acc0, l), d1 = lane_sums<TP>(acc1, l);
    if (l < T) {
      double c0 = __builtin_inf(), c1 = __builtin_inf();
      if (closest) {
        const double2 cv = *reinterpret_cast<const double2*>(closest + rb);  // rb is even, below stride
        c0 = cv.x;
        c1 = cv.y;
      }
      const double n0 = v0 ? (d0 < c0 ? d0 : c0) : 0.0;  // rows past B: zero, so the sums do not see them
      const double n1 = v1 ? (d1 < c1 ? d1 : c1) : 0.0;
      *reinterpret_cast<double2*>(out + (size_t)l * stride + rb) = make_double2(n0, n1);
      psum += n0;
      psum += n1;
    }
  }
  psum += __shfl_xor(psum, 16);
  psum += __shfl_xor(psum, 32);
  if (lane < 16) s_part[wave][lane] = psum;
  __syncthreads();
  if ((int)threadIdx.x < T) {
    const int t = threadIdx.x;
    part[(size_t)t * C + blockIdx.x] = ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
  }
}

QCE_DEV double read_lane(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// Lane i < n holds val_i.  Running sums base + val_0 + ... in ascending order (the last one replaced by `total` when
// snap); the first i whose sum is >= r: (idx, exc = the sum before it, inc = its sum) and true.  Else exc = the last
// sum and false.  Every lane of the wave takes part and gets the same answer.
QCE_DEV bool seq_search(double val, int n, double base, bool snap, double total, double r, int& idx, double& exc,
                        double& inc) {
  double acc = base;
  for (int i = 0; i < n; ++i) {
    const double nx = (snap && i == n - 1) ? total : acc + read_lane(val, i);
    if (nx >= r) {
      idx = i;
      exc = acc;
      inc = nx;
      return true;
    }
    acc = nx;
  }
  exc = acc;
  return false;
}

// part (Tprev, C) and scratch (Tprev, stride): the last candidate pass; cand_prev (Tprev): its candidate rows.
// Writes idx_out[0], pot_out[0] (the centre picked and the potential with it), win_out[0] (its scratch row) and, when
// Tn > 0, cand_next[t] for the trials u[t], t < Tn.
__global__ __launch_bounds__(1024) void k_km_seed_pick(int Tprev, int C, long long B, long long chunk, long long stride,
                                                        const double* __restrict__ part,
                                                        const double* __restrict__ scratch,
                                                        const long long* __restrict__ cand_prev,
                                                        const double* __restrict__ u, int Tn,
                                                        long long* __restrict__ idx_out, double* __restrict__ pot_out,
                                                        int* __restrict__ win_out, long long* __restrict__ cand_next) {
  __shared__ double s_g[16][KS_GROUP];
  __shared__ double s_pot[16];
  __shared__ int s_w;
  const int tid = threadIdx.x;
  const int NG = (C + KS_GROUP - 1) / KS_GROUP;  // <= 32
  if (tid < 16 * KS_GROUP) {
    const int t = tid >> 5, gl = tid & 31;
    double s = 0.0;
    if (t < Tprev && gl < NG) {
      const int c1 = (gl + 1) * KS_GROUP < C ? (gl + 1) * KS_GROUP : C;
      for (int c = gl * KS_GROUP; c < c1; ++c) s += part[(size_t)t * C + c];
    }
    s_g[t][gl] = s;
  }
  __syncthreads();
  if (tid < Tprev) {
    double s = 0.0;
    for (int gi = 0; gi < NG; ++gi) s += s_g[tid][gi];
    s_pot[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int w = 0;
    for (int t = 1; t < Tprev; ++t)
      if (s_pot[t] < s_pot[w]) w = t;  // the first minimum
    s_w = w;
    idx_out[0] = cand_prev[w];
    pot_out[0] = s_pot[w];
    win_out[0] = w;
  }
  __syncthreads();
  const int trial = tid >> 6, lane = tid & 63;
  if (trial >= Tn) return;  // uniform over the wave
  const int w = s_w;
  const double pot = s_pot[w];
  const double r = u[trial] * pot;
  long long j = B - 1;
  int gi = 0, ci = 0, si = 0, ri = 0;
  double gexc, ginc, cexc, cinc, sexc, sinc, rexc, rinc;
  if (seq_search(lane < NG ? s_g[w][lane] : 0.0, NG, 0.0, false, 0.0, r, gi, gexc, ginc)) {
    const int c0 = gi * KS_GROUP;
    const int nc = C - c0 < KS_GROUP ? C - c0 : KS_GROUP;
    seq_search(lane < nc ? part[(size_t)w * C + c0 + lane] : 0.0, nc, gexc, true, ginc, r, ci, cexc, cinc);
    const long long cs = (long long)(c0 + ci) * chunk;
    const double* row = scratch + (size_t)w * stride + cs;  // rows past B hold zeros
    const long long seg = chunk / KS_SEGS;
    double s = 0.0;
    for (long long k = 0; k < seg; ++k) s += row[lane * seg + k];
    seq_search(s, KS_SEGS, cexc, true, cinc, r, si, sexc, sinc);
    const long long j0 = si * seg;
    double acc = sexc;
    j = cs + j0 + seg - 1;
    for (long long wb = 0; wb < seg; wb += 64) {
      const int n = seg - wb < 64 ? (int)(seg - wb) : 64;
      if (seq_search(lane < n ? row[j0 + wb + lane] : 0.0, n, acc, wb + 64 >= seg, sinc, r, ri, rexc, rinc)) {
        j = cs + j0 + wb + ri;
        break;
      }
      acc = rexc;
    }
    if (j > B - 1) j = B - 1;
  }
  if (lane == 0) cand_next[trial] = j;
}

__global__ __launch_bounds__(256) void k_km_seed_gather(long long B, int N, int K, const double2* __restrict__ X,
                                                        const double2* __restrict__ mean,
                                                        const long long* __restrict__ idx,
                                                        double2* __restrict__ centers) {
  const long long n = (long long)K * N;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const long long k = e / N;
    const int c = (int)(e - k * N);
    long long j = idx[k];
    j = j < 0 ? 0 : j >= B ? B - 1 : j;
    const double2 x = X[j * N + c];
    centers[e] = mean ? csub(x, mean[c]) : x;
  }
}

template <int T>
hipError_t launch_cand(const QceKmSeedPlan& p, const double* X, const double* mean, const long long* cand,
                       const double* closest, const int* win, double* out, double* part, hipStream_t st) {
  const size_t lds = sizeof(double2) * (size_t)p.NP * (T + 1);
  if (lds > (32u << 10)) {
    hipError_t e = hipFuncSetAttribute((const void*)k_km_seed_cand<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_km_seed_cand<T>), dim3(p.C), dim3(256), lds, st, p.B, p.N, p.NP, p.chunk, p.stride, p.C,
                     reinterpret_cast<const double2*>(X), reinterpret_cast<const double2*>(mean), cand, closest, win,
                     out, part);
  return hipGetLastError();
}

}  // namespace

QceKmSeedPlan qce_km_seed_plan(long long B, int N) {
  QceKmSeedPlan p;
  p.B = B;
  p.N = N;
  p.NP = (N + 63) / 64 * 64;
  // at most 1024 chunks (32 groups of 32), each a multiple of 64 rows (64 segments; 32 rows per workgroup turn)
  const long long per = (B + 1023) / 1024;
  p.chunk = (per + 63) / 64 * 64;
  p.C = (int)((B + p.chunk - 1) / p.chunk);
  p.stride = p.chunk * p.C;
  return p;
}

hipError_t qce_launch_km_seed_cand(const QceKmSeedPlan& p, int T, const double* X, const double* mean,
                                   const long long* cand, const double* closest, const int* win, double* out,
                                   double* part, hipStream_t st) {
  switch (T) {
#define QCE_KS_CASE(t) \
  case t:              \
    return launch_cand<t>(p, X, mean, cand, closest, win, out, part, st);
    QCE_KS_CASE(1) QCE_KS_CASE(2) QCE_KS_CASE(3) QCE_KS_CASE(4) QCE_KS_CASE(5) QCE_KS_CASE(6) QCE_KS_CASE(7)
    QCE_KS_CASE(8) QCE_KS_CASE(9) QCE_KS_CASE(10) QCE_KS_CASE(11) QCE_KS_CASE(12) QCE_KS_CASE(13) QCE_KS_CASE(14)
    QCE_KS_CASE(15) QCE_KS_CASE(16)
#undef QCE_KS_CASE
  }
  return hipErrorInvalidValue;
}

hipError_t qce_launch_km_seed_pick(const QceKmSeedPlan& p, int Tprev, const double* part, const double* scratch,
                                   const long long* cand_prev, const double* u, int Tn, long long* idx_out,
                                   double* pot_out, int* win_out, long long* cand_next, hipStream_t st) {
  if (Tprev < 1 || Tprev > 16 || Tn < 0 || Tn > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_km_seed_pick, dim3(1), dim3(1024), 0, st, Tprev, p.C, p.B, p.chunk, p.stride, part, scratch,
                     cand_prev, u, Tn, idx_out, pot_out, win_out, cand_next);
  return hipGetLastError();
}

hipError_t qce_launch_km_seed_gather(const QceKmSeedPlan& p, int K, const double* X, const double* mean,
                                     const long long* idx, double* centers, hipStream_t st) {
  long long g = ((long long)K * p.N + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_km_seed_gather, dim3((unsigned)g), dim3(256), 0, st, p.B, p.N, K,
                     reinterpret_cast<const double2*>(X), reinterpret_cast<const double2*>(mean), idx,
                     reinterpret_cast<double2*>(centers));
  return hipGetLastError();
}
