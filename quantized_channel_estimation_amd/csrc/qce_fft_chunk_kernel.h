// k_fft_chunk: the MFMA Fourier estimate kernel for zero-mean models at N = 128, 256, and its launcher.
#pragma once
#include "qce_fft_dev.h"

FW_STAMP_UNIT(qce_fft_chunk_set_stamps)

namespace {

// Zero-mean models, N = 128, 256: one workgroup (4 waves) per 16 observations, the components split over the waves
// for the log-probabilities and the bins split over the waves for the filter, so the softmax of every (component,
// observation) is evaluated exactly once and the waves meet at two barriers per chunk of 128 components (not per
// block of 16).  Per chunk:
//   lp    wave w: blocks w, w + 4 of the chunk over all N bins: D[comp][obs] = c'_comp + sum_bins (-rinv) |Y|^2
//         (A: fragment-order table from L2, B: |Y|^2 from LDS, both blocks share each B read)
//   max   per-wave column max -> LDS, barrier, every wave takes the chunk max (fixed order) and the running max
//   e     e = exp(lp - m) of the wave's own 32 components -> LDS (the filter's B layout), column sums -> LDS, barrier
//   F     wave w: its N/4 bins over the chunk's 128 components: F[bin][obs] = alpha F + w[comp][bin] e[comp][obs]
// Layout: the spectra tile T (16 x (N+1) complex) carries the y load and the forward FFT; the lane's filter-phase
// spectra (bins bin0 + 16 t + hq + 4 r) move to registers and the tile is reused for |Y|^2 (in the lp B layout),
// e and the per-wave column maxima / sums; after the last chunk it takes Z = Y f for the inverse FFT.
template <int N>
struct FftChunkLds {
  static constexpr int TS = 16, RS = N + 1;
  static constexpr size_t tile = (size_t)TS * RS * 16;
  static constexpr size_t y2 = (size_t)N * TS * 8, e = (size_t)128 * TS * 8, sm = (size_t)2 * 4 * TS * 8;
  static constexpr size_t body = tile > y2 + e + sm ? tile : y2 + e + sm;
  static constexpr size_t bytes = 128 * 16 + body + 32 * 8 + 64 * 16;  // + the exp table, the pass-1 lane twiddles
};

template <int N, int OUT>
__global__ __launch_bounds__(256, 2) void k_fft_chunk(long long B, int lg1, int lg2, int Kp,
                                                      const double2* __restrict__ y, const double* __restrict__ pr,
                                                      const double* __restrict__ pc, const double* __restrict__ pw,
                                                      double2* __restrict__ h, double* __restrict__ om,
                                                      double* __restrict__ os, float* __restrict__ oa) {
  constexpr int TS = 16, RS = N + 1, lgTS = 4;
  constexpr int lgN = __builtin_ctz(N);
  constexpr int NB = N / 4;    // bins per wave in the filter product
  constexpr int NTW = NB / 16;  // the wave's 16-bin filter tiles
  constexpr int NTF = N / 16;   // 16-bin tiles of the whole filter table
  constexpr int NL = N / 8;     // 16-byte lp operand loads per block (two k-steps each)
  constexpr int NWF = N / 8;    // 16-byte filter operand loads per block
  constexpr int CB = 8;         // component blocks per chunk (two per wave)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* tw = reinterpret_cast<double2*>(smem);
  double2* T = tw + 128;
  double2* Y2 = T;                                                 // [N/8][4][16] (k-steps 2i, 2i+1 of the lp B)
  double2* E = reinterpret_cast<double2*>(reinterpret_cast<double*>(T) + N * TS);  // [CB * 2][4][16]
  double* SM = reinterpret_cast<double*>(E + CB * 2 * 64);         // [2][4][16] column maxima, column sums
  double* etab = reinterpret_cast<double*>(smem) + 2 * 128 + FftChunkLds<N>::body / 8;  // 2^(j/32), after the body
  double2* tl = reinterpret_cast<double2*>(etab + 32);                                  // pass-1 lane twiddles (N = 256)
  const int tid = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * TS;
  const int rows = (int)((B - b0) < TS ? (B - b0) : TS);
  FW_STAMP_DECL

  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int col = lane & 15, hq = lane >> 4;
  const int bin0 = wid * NB;
  double2 yv[NTW * 4];  // the lane's filter-phase spectra (tile t, accumulator row hq + 4 r: yv[4 t + r])
  if constexpr (N == 256) {
    // pass 1 straight from HBM: thread (s = tid / 16, g = tid % 16) holds positions g + 16 i of observation s (each
    // i a 256-byte contiguous run over 16 lanes); pass 2 thread (wave w, hq, col) the positions 16 (hq + 4 w) + i of
    // observation col, which stay in registers as yv
    const int s1 = tid >> 4, g = tid & 15;
    {
      const double2* yr = y + (b0 + (s1 < rows ? s1 : rows - 1)) * N + g;
      double2 x[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = yr[16 * i];
      for (int t = tid; t < 128; t += 256) {
        double sn, cs;
        sincospi(-(double)t / 128.0, &sn, &cs);
        tw[t] = make_double2(cs, sn);
      }
      exp2_tab_init(etab, tid);
      pass1_lane_tw(tl, 8, lg2, tid);
      __syncthreads();
      FW_STAMP(0);
      if (s1 >= rows) {
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = make_double2(0.0, 0.0);
      }
      fft256_pass1<false>(x, lg2, g, tl);
#pragma unroll
      for (int i = 0; i < 16; ++i) T[s1 * RS + g + 16 * i] = x[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) yv[i] = T[col * RS + 16 * (hq + 4 * wid) + i];
    fft_pass_low4<false>(yv, lg2, tw);
    FW_STAMP(1);
    __syncthreads();  // every spectrum value is in registers: the tile takes |Y|^2, e and the column statistics
    // |Y|^2 in the lp B layout (k-step u = p / 4 covers p = 4 u + hq'): position 16 (hq + 4 w) + r + 4 t is k-step
    // u = 4 (hq + 4 w) + t, row hq' = r; the pair (t even, t odd) is one 16-byte slot
#pragma unroll
    for (int tp = 0; tp < 2; ++tp)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 a = yv[r + 8 * tp], b = yv[r + 8 * tp + 4];
        Y2[((2 * (hq + 4 * wid) + tp) * 4 + r) * 16 + col] =
            make_double2(a.x * a.x + a.y * a.y, b.x * b.x + b.y * b.y);
      }
    __syncthreads();
  } else {
    for (int t = tid; t < 128; t += 256) {
      double sn, cs;
      sincospi(-(double)t / 128.0, &sn, &cs);
      tw[t] = make_double2(cs, sn);
    }
    exp2_tab_init(etab, tid);
    {  // all loads in flight at once; rows past the batch end read a clamped (valid) row and are stored as 0
      constexpr int NLY = TS * N / 256;
      const double2* yt = y + b0 * N;
      double2 v[NLY];
#pragma unroll
      for (int i = 0; i < NLY; ++i) {
        const int e = tid + 256 * i, r = e >> lgN;
        v[i] = yt[(r < rows ? r : rows - 1) * N + (e & (N - 1))];
      }
#pragma unroll
      for (int i = 0; i < NLY; ++i) {
        const int e = tid + 256 * i, r = e >> lgN;
        T[r * RS + (e & (N - 1))] = (r < rows) ? v[i] : make_double2(0.0, 0.0);
      }
    }
    __syncthreads();
    FW_STAMP(0);
    fft_axis_passes<false>(T, lgTS, RS, lgN, lg2, 1, tw);
    if (lg1 > 0) fft_axis_passes<false>(T, lgTS, RS, lgN, lg1, 1 << lg2, tw);
    FW_STAMP(1);
    // bin bin0 + 16 t + hq + 4 r, observation col
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) yv[4 * t + r] = T[col * RS + bin0 + 16 * t + hq + 4 * r];
    {  // |Y|^2 in the lp B layout: pair (k-step 2i, 2i + 1) of lane (hq, col) = bins 8 i + hq, 8 i + 4 + hq
      constexpr int NP = N * TS / 2 / 256;
      double2 q[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int p = tid + 256 * j, s = p & 15, rest = p >> 4;
        const int bq = 8 * (rest >> 2) + (rest & 3);
        const double2 a = T[s * RS + bq], b = T[s * RS + bq + 4];
        q[j] = make_double2(a.x * a.x + a.y * a.y, b.x * b.x + b.y * b.y);
      }
      __syncthreads();  // every spectrum value is in registers: the tile takes |Y|^2, e and the column statistics
#pragma unroll
      for (int j = 0; j < NP; ++j) Y2[tid + 256 * j] = q[j];  // index = (i * 4 + hq) * 16 + s
      __syncthreads();
    }
  }
  FW_STAMP(2);

  f64x4 F[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t)
    for (int r = 0; r < 4; ++r) F[t][r] = 0.0;
  double m = -__builtin_inf(), ssum = 0.0;
  const int ncb = Kp >> 4;
  // tables through buffer descriptors: scalar block offsets, one 32-bit lane offset (no 64-bit address math)
  const __amdgpu_buffer_rsrc_t rpr = buf_rsrc(pr, (unsigned)(Kp * N * 8)), rpw = buf_rsrc(pw, (unsigned)(Kp * N * 8));
  const unsigned ul16 = (unsigned)lane * 16;
  const double2* Y2l = Y2 + hq * 16 + col;
  for (int c0 = 0; c0 < ncb; c0 += CB) {
    const int cb0 = c0 + wid, cb1 = cb0 + 4;
    const bool v0 = cb0 < ncb, v1 = cb1 < ncb;  // wave-uniform
    f64x4 C0, C1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      C0[r] = v0 ? pc[16 * cb0 + hq + 4 * r] : -__builtin_inf();
      C1[r] = v1 ? pc[16 * cb1 + hq + 4 * r] : -__builtin_inf();
    }
    if (v1) {
      const unsigned o0 = (unsigned)cb0 * NL * 1024, o1 = (unsigned)cb1 * NL * 1024;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double2 a0 = buf_ld2(rpr, ul16, o0 + 1024 * i), a1 = buf_ld2(rpr, ul16, o1 + 1024 * i), b = Y2l[i * 64];
        C0 = mfma16x16x4d(a0.x, b.x, C0);
        C1 = mfma16x16x4d(a1.x, b.x, C1);
        C0 = mfma16x16x4d(a0.y, b.y, C0);
        C1 = mfma16x16x4d(a1.y, b.y, C1);
      }
    } else if (v0) {
      const unsigned o0 = (unsigned)cb0 * NL * 1024;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double2 a0 = buf_ld2(rpr, ul16, o0 + 1024 * i), b = Y2l[i * 64];
        C0 = mfma16x16x4d(a0.x, b.x, C0);
        C0 = mfma16x16x4d(a0.y, b.y, C0);
      }
    }
    FW_STAMP(3);
    // chunk maximum per observation: per-wave column maxima, then all four in a fixed order
    const double lm = col_max4(fmax(fmax(fmax(C0[0], C0[1]), fmax(C0[2], C0[3])),
                                    fmax(fmax(C1[0], C1[1]), fmax(C1[2], C1[3]))));
    if (hq == 0) SM[wid * 16 + col] = lm;
    __syncthreads();
    const double mn = fmax(fmax(m, fmax(SM[col], SM[16 + col])), fmax(SM[32 + col], SM[48 + col]));
    const double sh = (mn == -__builtin_inf()) ? 0.0 : mn;
    const double alpha = exp_nonpos(m - sh, etab);
    // e of the wave's own components, in the filter's B layout: k-step ks = 4 (local block) + r covers the
    // components 4 ks + hq; pair (ks even, ks + 1) per 16-byte slot
    double ls = 0.0;
    {
      double e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = v0 ? exp_nonpos(C0[r] - sh, etab) : 0.0;
      ls += (e[0] + e[1]) + (e[2] + e[3]);
      E[((2 * wid) * 4 + hq) * 16 + col] = make_double2(e[0], e[1]);
      E[((2 * wid + 1) * 4 + hq) * 16 + col] = make_double2(e[2], e[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = v1 ? exp_nonpos(C1[r] - sh, etab) : 0.0;
      ls += (e[0] + e[1]) + (e[2] + e[3]);
      E[((2 * (wid + 4)) * 4 + hq) * 16 + col] = make_double2(e[0], e[1]);
      E[((2 * (wid + 4) + 1) * 4 + hq) * 16 + col] = make_double2(e[2], e[3]);
    }
    ls = col_sum4(ls);
    if (hq == 0) SM[64 + wid * 16 + col] = ls;
    __syncthreads();
    ssum = ssum * alpha + ((SM[64 + col] + SM[80 + col]) + (SM[96 + col] + SM[112 + col]));
    m = mn;
    FW_STAMP(4);
#pragma unroll
    for (int t = 0; t < NTW; ++t) F[t] *= alpha;
    // filter over the chunk's blocks (padding blocks beyond ncb carry e = 0 and are skipped)
    // the operands of block bl + 1 are fetched while block bl computes; the CB blocks are unrolled (guards are
    // wave-uniform), so the two operand buffers alternate without register copies
    const int nbl = (ncb - c0) < CB ? (ncb - c0) : CB;
    constexpr int NWL = 2 * NTW;  // 16-byte filter operand loads per block and wave: (r, tile pair tp)
    const unsigned wbase = (unsigned)c0 * NWF * 1024 + (unsigned)((wid * NTW) >> 1) * 1024;
    auto load_w = [&](int bl, double2 (&wv)[NWL]) {
      const unsigned ob = wbase + (unsigned)bl * NWF * 1024;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int tp = 0; tp < NTW / 2; ++tp)
          wv[r * (NTW / 2) + tp] = buf_ld2(rpw, ul16, ob + ((r * NTF) >> 1) * 1024 + tp * 1024);
    };
    auto filter_blk = [&](int bl, const double2 (&wc)[NWL]) {
#pragma unroll
      for (int rp = 0; rp < 2; ++rp) {
        const double2 ev = E[((2 * bl + rp) * 4 + hq) * 16 + col];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int r = 2 * rp + rr;
          const double eb = rr ? ev.y : ev.x;
#pragma unroll
          for (int tp = 0; tp < NTW / 2; ++tp) {  // filter table pair (j, j + 1), j = r NTF + t: tiles t, t + 1
            const double2 wv = wc[r * (NTW / 2) + tp];
            F[2 * tp] = mfma16x16x4d(wv.x, eb, F[2 * tp]);
            F[2 * tp + 1] = mfma16x16x4d(wv.y, eb, F[2 * tp + 1]);
          }
        }
      }
    };
    double2 wa[NWL], wb[NWL];
    load_w(0, wa);
#pragma unroll
    for (int bl = 0; bl < CB; bl += 2) {
      if (bl < nbl) {
        if (bl + 1 < nbl) load_w(bl + 1, wb);
        filter_blk(bl, wa);
      }
      if (bl + 1 < nbl) {
        if (bl + 2 < nbl) load_w(bl + 2, wa);
        filter_blk(bl + 1, wb);
      }
    }
    FW_STAMP(5);
  }
  __syncthreads();  // every wave is done with |Y|^2 and e: the tile takes Z
  const double sc = (OUT == 0) ? 1.0 / ssum : 1.0;
  if ((OUT == 3 || OUT == 4) && wid == 0 && hq == 0 && col < rows) {
    om[b0 + col] = m;
    os[b0 + col] = ssum;
  }
  if constexpr (N == 256) {  // inverse pass 2 on the registers, one LDS exchange, inverse pass 1, store from registers
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double f = F[t][r] * sc;
        yv[4 * t + r] = make_double2(yv[4 * t + r].x * f, yv[4 * t + r].y * f);
      }
    fft_pass_low4<true>(yv, lg2, tw);
#pragma unroll
    for (int i = 0; i < 16; ++i) T[col * RS + 16 * (hq + 4 * wid) + i] = yv[i];
    __syncthreads();
    const int s1 = tid >> 4, g = tid & 15;
    double2 x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = T[s1 * RS + g + 16 * i];
    fft256_pass1<true>(x, lg2, g, tl);
    FW_STAMP(6);
    if (s1 < rows) {
      const long long o = (b0 + s1) * N + g;
      if (OUT == 3) {
        float2* at = reinterpret_cast<float2*>(oa) + o;
#pragma unroll
        for (int i = 0; i < 16; ++i) at[16 * i] = make_float2((float)x[i].x, (float)x[i].y);
      } else if (OUT == 4) {
        double2* at = reinterpret_cast<double2*>(oa) + o;
#pragma unroll
        for (int i = 0; i < 16; ++i) at[16 * i] = x[i];
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) h[o + 16 * i] = x[i];
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 v = yv[4 * t + r];
        const double f = F[t][r] * sc;
        T[col * RS + bin0 + 16 * t + hq + 4 * r] = make_double2(v.x * f, v.y * f);
      }
    __syncthreads();
    if (lg1 > 0) fft_axis_passes<true>(T, lgTS, RS, lgN, lg1, 1 << lg2, tw);
    fft_axis_passes<true>(T, lgTS, RS, lgN, lg2, 1, tw);
    FW_STAMP(6);
    if (OUT == 3) {
      float2* at = reinterpret_cast<float2*>(oa) + b0 * N;
#pragma unroll 4
      for (int e = tid; e < rows * N; e += 256) {
        const double2 v = T[(e >> lgN) * RS + (e & (N - 1))];
        at[e] = make_float2((float)v.x, (float)v.y);
      }
    } else if (OUT == 4) {
      double2* at = reinterpret_cast<double2*>(oa) + b0 * N;
#pragma unroll 4
      for (int e = tid; e < rows * N; e += 256) at[e] = T[(e >> lgN) * RS + (e & (N - 1))];
    } else if (rows == TS) {
      double2* ht = h + b0 * N;
      constexpr int NLY = TS * N / 256;
      double2 v[NLY];
#pragma unroll
      for (int i = 0; i < NLY; ++i) {
        const int e = tid + 256 * i;
        v[i] = T[(e >> lgN) * RS + (e & (N - 1))];
      }
#pragma unroll
      for (int i = 0; i < NLY; ++i) ht[tid + 256 * i] = v[i];
    } else {
      double2* ht = h + b0 * N;
#pragma unroll 4
      for (int e = tid; e < rows * N; e += 256) ht[e] = T[(e >> lgN) * RS + (e & (N - 1))];
    }
  }
  FW_STAMP(7);
  FW_STAMP_FLUSH
}

template <int N, int OUT>
hipError_t launch_chunk_t(const QceFftEstArgs& a, hipStream_t st) {
  constexpr size_t lds = FftChunkLds<N>::bytes;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fft_chunk<N, OUT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int lg1 = __builtin_ctz(a.n1), lg2 = __builtin_ctz(a.n2);
  dim3 grid((unsigned)((a.B + 15) / 16));
  hipLaunchKernelGGL((k_fft_chunk<N, OUT>), grid, dim3(256), lds, st, a.B, lg1, lg2, a.Kp, a.y, a.pr, a.pc, a.pw,
                     a.h, a.om, a.os, a.oa);
  return hipGetLastError();
}

}  // namespace
