// k_fft_wave: the MFMA Fourier estimate kernel for N = 16, 32 (wave-local LDS transform), and its launcher.
#pragma once
#include "qce_fft_dev.h"

FW_STAMP_UNIT(qce_fft_wave_set_stamps)

namespace {

// N <= 32: one wave owns 16 observations end to end (load, FFT, both products, IFFT, store) with no
// workgroup barrier after the twiddle table; waves loop over 16-observation tiles (persistent grid of
// two workgroups per CU, 8 waves per CU).  The spectra stay in the wave's LDS tile through the component
// loop, |Y|^2 in registers.  Tables are in fragment order (k_fft_pack): a lane's operands for two
// consecutive MFMAs are one 16-byte load, and block cb+1's operands are fetched while block cb computes.
//   lp  table: [cb][t/2][lane][t&1] = -rinv[bin 4t + lane/16][comp 16cb + lane%16]       t < N/4
//   filter   : [cb][j/2][lane][j&1] = w[comp 16cb + lane/16 + 4r][bin 16t + lane%16]     j = r NT + t
// CIRC: one axis (n1 = 1, circulant), FFT passes resolved at compile time
template <int N, int OUT, bool HM, bool CIRC>
__global__ __launch_bounds__(256, HM ? 1 : 2) void k_fft_wave(long long B, long long ntiles, int lg1, int lg2, int Kp,
                                                     const double2* __restrict__ y, const double* __restrict__ pr,
                                                     const double* __restrict__ pur, const double* __restrict__ pui,
                                                     const double* __restrict__ pc, const double* __restrict__ pw,
                                                     const double* __restrict__ pbr, const double* __restrict__ pbi,
                                                     double2* __restrict__ h, double* __restrict__ om,
                                                     double* __restrict__ os, float* __restrict__ oa) {
  constexpr int NT = N / 16;  // 16-bin tiles of the filter product
  constexpr int NK = N / 4;   // k-steps of the lp product
  constexpr int NL = NK / 2;  // 16-byte lp operand loads per block
  constexpr int NW = 2 * NT;  // 16-byte filter operand loads per block
  constexpr int RS = N + 1;
  constexpr int lgN = __builtin_ctz(N);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* tw = reinterpret_cast<double2*>(smem);
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  double2* T = tw + 128 + wid * (16 * RS);
  for (int t = tid; t < 128; t += 256) {
    double sn, cs;
    sincospi(-(double)t / 128.0, &sn, &cs);
    tw[t] = make_double2(cs, sn);
  }
  __syncthreads();
  const int col = lane & 15, hq = lane >> 4;
  double2* Trow = T + col * RS;
  const int ncb = Kp >> 4;
  const double2* PR = reinterpret_cast<const double2*>(pr) + lane;
  const double2* PW = reinterpret_cast<const double2*>(pw) + lane;
  FW_STAMP_DECL
  // Main phase: whole rounds of tiles, one wave per tile.  The remainder (fewer tiles than waves: the last,
  // partial round at large B, every tile at small B) is worked by the four waves of a workgroup together,
  // each on every fourth component block, with the partial (m, s, F) merged through LDS (zero-mean models)
  const long long W = (long long)gridDim.x * 4;
  const long long nmain = HM ? ntiles : (ntiles / W) * W;
  // y of the wave's next tile is fetched into registers behind the component loop of the current one
  // (N/4 16-byte loads in flight, latency hidden by the filter epilogue, inverse FFT and store); rows
  // past the batch end read a clamped (valid) row and are stored as 0
  double2 v[N / 4];
  auto load_y = [&](long long t) __attribute__((always_inline)) {
    const long long bb = t * 16;
    const int rr = (int)((B - bb) < 16 ? (B - bb) : 16);
    const double2* yt = y + bb * N;
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const int e = lane + 64 * i, r = e >> lgN;
      v[i] = yt[(r < rr ? r : rr - 1) * N + (e & (N - 1))];
    }
  };
  constexpr bool PREF = !HM;  // the mean terms' accumulators leave no registers for the prefetch
  // one tile: component blocks s0, s0 + bs, ...; next >= 0: prefetch that tile's y (main phase);
  // coop: the workgroup's four waves share the tile (bs = 4), wave 0 merges and writes
  auto run_tile = [&](long long tile, int s0, int bs, long long next, bool coop) __attribute__((always_inline)) {
    const long long b0 = tile * 16;
    const int rows = (int)((B - b0) < 16 ? (B - b0) : 16);
    if (!PREF || coop) load_y(tile);
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const int e = lane + 64 * i, r = e >> lgN;
      T[r * RS + (e & (N - 1))] = (r < rows) ? v[i] : make_double2(0.0, 0.0);
    }
    wave_lds_sync();
    FW_STAMP(0);
    if constexpr (CIRC) {
      fft_axis_passes<false, true>(T, 4, RS, lgN, lgN, 1, tw);  // compile-time passes and indices
    } else {
      fft_axis_passes<false, true>(T, 4, RS, lgN, lg2, 1, tw);
      if (lg1 > 0) fft_axis_passes<false, true>(T, 4, RS, lgN, lg1, 1 << lg2, tw);
    }
    FW_STAMP(1);
    // |Y|^2 (the lp B operand) is re-derived from the spectra in LDS per block instead of held in 2 N / 4
    // registers: those registers carry the next tile's y instead
    auto y2 = [&](int t) {
      const double2 q = Trow[4 * t + hq];
      return q.x * q.x + q.y * q.y;
    };
    f64x4 F[NT], Br[HM ? NT : 1], Bi[HM ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      for (int r = 0; r < 4; ++r) F[t][r] = 0.0;
    if constexpr (HM) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 4; ++r) Br[t][r] = Bi[t][r] = 0.0;
    }
    double m = -__builtin_inf(), ssum = 0.0;
    // Software pipeline over component blocks: iteration j issues the lp MFMAs of block j+1 (independent
    // of block j's softmax VALU, so the two overlap), then block j's softmax and filter MFMAs.
    auto lp_block = [&](int cb, const double2* ta, const double* pcv) {
      f64x4 C;
#pragma unroll
      for (int r = 0; r < 4; ++r) C[r] = pcv[r];
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        C = mfma16x16x4d(ta[i].x, y2(2 * i), C);
        C = mfma16x16x4d(ta[i].y, y2(2 * i + 1), C);
      }
      if constexpr (HM) {
        const double2* qa = reinterpret_cast<const double2*>(pur) + lane + cb * NL * 64;
        const double2* qb = reinterpret_cast<const double2*>(pui) + lane + cb * NL * 64;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const double2 ua = qa[i * 64], ub = qb[i * 64];
          const double2 v0 = Trow[8 * i + hq], v1 = Trow[8 * i + 4 + hq];
          C = mfma16x16x4d(ua.x, v0.x, C);
          C = mfma16x16x4d(ub.x, v0.y, C);
          C = mfma16x16x4d(ua.y, v1.x, C);
          C = mfma16x16x4d(ub.y, v1.y, C);
        }
      }
      return C;
    };
    // online softmax over one block of 16 components (rows hq + 4 r, all four lane groups of a column);
    // branch-free: an all -inf prefix gives alpha = e = 0 through the 0 shift
    auto softmax = [&](const f64x4& C, double* e) {
      const double bm = col_max4(fmax(fmax(C[0], C[1]), fmax(C[2], C[3])));
      const double mn = fmax(m, bm);
      const double sh = (mn == -__builtin_inf()) ? 0.0 : mn;
      const double alpha = exp(m - sh);
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = exp(C[r] - sh);
      const double ls = col_sum4((e[0] + e[1]) + (e[2] + e[3]));
      ssum = ssum * alpha + ls;
      m = mn;
      return alpha;
    };
    auto filter_block = [&](int cb, const double2* tb, const double* e, double alpha) {
#pragma unroll
      for (int t = 0; t < NT; ++t) F[t] *= alpha;
#pragma unroll
      for (int j = 0; j < 4 * NT; ++j) {
        const int r = j / NT, t = j % NT;
        const double wv = (j & 1) ? tb[j >> 1].y : tb[j >> 1].x;
        F[t] = mfma16x16x4d(wv, e[r], F[t]);
      }
      if constexpr (HM) {
        const double2* qa = reinterpret_cast<const double2*>(pbr) + lane + cb * NW * 64;
        const double2* qb = reinterpret_cast<const double2*>(pbi) + lane + cb * NW * 64;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          Br[t] *= alpha;
          Bi[t] *= alpha;
        }
#pragma unroll
        for (int j = 0; j < 4 * NT; ++j) {
          const int r = j / NT, t = j % NT;
          const double2 ua = qa[(j >> 1) * 64], ub = qb[(j >> 1) * 64];
          Br[t] = mfma16x16x4d((j & 1) ? ua.y : ua.x, e[r], Br[t]);
          Bi[t] = mfma16x16x4d((j & 1) ? ub.y : ub.x, e[r], Bi[t]);
        }
      }
    };
    const int nb = (ncb - s0 + bs - 1) / bs;  // this wave's component blocks s0 + j bs, j < nb
    auto blk = [&](int j) { return s0 + j * bs; };
    if (nb > 0) {
      const int last = nb - 1;
      double2 ta[NL], tb[NW];
      double pcv[4];
#pragma unroll
      for (int i = 0; i < NL; ++i) ta[i] = PR[(blk(0) * NL + i) * 64];
#pragma unroll
      for (int r = 0; r < 4; ++r) pcv[r] = pc[16 * blk(0) + hq + 4 * r];
      f64x4 C = lp_block(blk(0), ta, pcv);
      {
        const int b1 = blk(last > 0 ? 1 : 0);
#pragma unroll
        for (int i = 0; i < NL; ++i) ta[i] = PR[(b1 * NL + i) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) pcv[r] = pc[16 * b1 + hq + 4 * r];
#pragma unroll
        for (int i = 0; i < NW; ++i) tb[i] = PW[(blk(0) * NW + i) * 64];
      }
      FW_STAMP(2);
      // operand registers are refilled right after the MFMAs that read them: lp operands of block j+2
      // behind the lp MFMAs of j+1, filter operands of j+1 behind the filter MFMAs of j
      for (int j = 0; j < last; ++j) {
        const int b1 = blk(j + 1), b2 = blk(j + 2 < last ? j + 2 : last);
        const f64x4 Cn = lp_block(b1, ta, pcv);
#pragma unroll
        for (int i = 0; i < NL; ++i) ta[i] = PR[(b2 * NL + i) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) pcv[r] = pc[16 * b2 + hq + 4 * r];
        double e[4];
        const double alpha = softmax(C, e);
        filter_block(blk(j), tb, e, alpha);
#pragma unroll
        for (int i = 0; i < NW; ++i) tb[i] = PW[(b1 * NW + i) * 64];
        C = Cn;
      }
      FW_STAMP(3);
      if (PREF && next >= 0) {
        load_y(next);
      } else {  // define v on every path, so the consumed values are dead through the component loop
#pragma unroll
        for (int i = 0; i < N / 4; ++i) v[i] = make_double2(0.0, 0.0);
      }
      {
        double e[4];
        const double alpha = softmax(C, e);
        filter_block(blk(last), tb, e, alpha);
      }
    }
    if (coop) {  // waves 1-3 hand (F, m, s) to wave 0 through their own (now free) spectra tiles
      double* Td = reinterpret_cast<double*>(T);
      if (wid != 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) Td[(t * 4 + r) * 64 + lane] = F[t][r];
        Td[4 * NT * 64 + lane] = m;
        Td[(4 * NT + 1) * 64 + lane] = ssum;
      }
      __syncthreads();
      if (wid == 0) {  // fixed order: wave 0's own partial, then waves 1, 2, 3
        double mm = m;
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const double* Tw = reinterpret_cast<const double*>(tw + 128 + w * (16 * RS));
          mm = fmax(mm, Tw[4 * NT * 64 + lane]);
        }
        const double f0 = exp(m - mm);
        ssum *= f0;
#pragma unroll
        for (int t = 0; t < NT; ++t) F[t] *= f0;
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const double* Tw = reinterpret_cast<const double*>(tw + 128 + w * (16 * RS));
          const double mw = Tw[4 * NT * 64 + lane];
          const double fw = (mw == -__builtin_inf()) ? 0.0 : exp(mw - mm);
          ssum = fma(Tw[(4 * NT + 1) * 64 + lane], fw, ssum);
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) F[t][r] = fma(Tw[(t * 4 + r) * 64 + lane], fw, F[t][r]);
        }
        m = mm;
      }
    }
    if (!coop || wid == 0) {
      // Z = Y f + bb in place (each (observation, bin) of the tile belongs to exactly one lane)
      const double sc = (OUT == 0) ? 1.0 / ssum : 1.0;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bin = 16 * t + hq + 4 * r;
          const double2 q = Trow[bin];
          const double f = F[t][r] * sc;
          if constexpr (HM)
            Trow[bin] = make_double2(fma(q.x, f, Br[t][r] * sc), fma(q.y, f, Bi[t][r] * sc));
          else
            Trow[bin] = make_double2(q.x * f, q.y * f);
        }
      if ((OUT == 3 || OUT == 4) && hq == 0 && col < rows) {
        om[b0 + col] = m;
        os[b0 + col] = ssum;
      }
      FW_STAMP(4);
      wave_lds_sync();
      if constexpr (CIRC) {
        fft_axis_passes<true, true>(T, 4, RS, lgN, lgN, 1, tw);
      } else {
        if (lg1 > 0) fft_axis_passes<true, true>(T, 4, RS, lgN, lg1, 1 << lg2, tw);
        fft_axis_passes<true, true>(T, 4, RS, lgN, lg2, 1, tw);
      }
      FW_STAMP(5);
      if (OUT == 3) {
        float2* at = reinterpret_cast<float2*>(oa) + b0 * N;
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
          const int e = lane + 64 * i, r = e >> lgN;
          if (r < rows) {
            const double2 q = T[r * RS + (e & (N - 1))];
            at[e] = make_float2((float)q.x, (float)q.y);
          }
        }
      } else if (OUT == 4) {
        double2* at = reinterpret_cast<double2*>(oa) + b0 * N;
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
          const int e = lane + 64 * i, r = e >> lgN;
          if (r < rows) at[e] = T[r * RS + (e & (N - 1))];
        }
      } else {
        double2* ht = h + b0 * N;
        if (rows == 16) {  // whole tile: no per-element guard, all LDS reads issued before the stores
#pragma unroll
          for (int i = 0; i < N / 4; ++i) {
            const int e = lane + 64 * i;
            ht[e] = T[(e >> lgN) * RS + (e & (N - 1))];
          }
        } else {
#pragma unroll
          for (int i = 0; i < N / 4; ++i) {
            const int e = lane + 64 * i, r = e >> lgN;
            if (r < rows) ht[e] = T[r * RS + (e & (N - 1))];
          }
        }
      }
    }
    if (coop) __syncthreads();  // wave 0 has read the partials before the next tile overwrites them
    FW_STAMP(6);
    wave_lds_sync();
  };
  long long tile = (long long)blockIdx.x * 4 + wid;
  if (PREF && tile < nmain) load_y(tile);
  for (; tile < nmain; tile += W) run_tile(tile, 0, 1, tile + W < nmain ? tile + W : -1, false);
  for (long long tt = nmain + blockIdx.x; tt < ntiles; tt += gridDim.x) run_tile(tt, wid, 4, -1, true);
  FW_STAMP_FLUSH
}

template <int N, int OUT, bool HM, bool CIRC>
hipError_t launch_wave_c(const QceFftEstArgs& a, hipStream_t st) {
  const size_t lds = 128 * 16 + (size_t)4 * 16 * (N + 1) * 16;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fft_wave<N, OUT, HM, CIRC>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int lg1 = __builtin_ctz(a.n1), lg2 = __builtin_ctz(a.n2);
  const long long ntiles = (a.B + 15) / 16;
  // persistent: two workgroups (8 waves) per CU; with means one (their accumulators need the registers of
  // two waves)
  const long long slots = (HM ? 1LL : 2LL) * (a.cu > 0 ? a.cu : 256);
  // zero-mean: one workgroup per tile up to the slot count (tiles beyond whole rounds of 4 waves are
  // worked cooperatively by a workgroup's four waves); with means: one wave per tile
  const long long want = HM ? (ntiles + 3) / 4 : ntiles;
  const long long wgs = want < slots ? want : slots;
  hipLaunchKernelGGL((k_fft_wave<N, OUT, HM, CIRC>), dim3((unsigned)wgs), dim3(256), lds, st, a.B, ntiles, lg1, lg2,
                     a.Kp, a.y, a.pr, a.pur, a.pui, a.pc, a.pw, a.pbr, a.pbi, a.h, a.om, a.os, a.oa);
  return hipGetLastError();
}

}  // namespace
