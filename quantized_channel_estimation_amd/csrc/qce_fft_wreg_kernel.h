// k_fft_wreg: the MFMA Fourier estimate kernel for N = 64 (register transform), and its launcher.
#pragma once
#include "qce_fft_dev.h"

FW_STAMP_UNIT(qce_fft_wreg_set_stamps)

namespace {

// Zero-mean models, N = 64 (cfg3): k_fft_wave's persistent one-wave-per-tile schedule with the transform in registers.
// Pass 1 (storage bits 5, 4) runs on the prefetched y (lane: observations s0 + 4 q, positions g + 16 j), one
// wave-local LDS exchange, pass 2 (bits 3..0) leaves lane (hq, col) holding positions 16 hq + i of observation col.
// The tables are ordered so those 16 points are the lane's own operands: lp k-step u, k-index hq = position
// 16 hq + u (the B operand |Y|^2 comes from registers, computed once per tile), filter tile t, row hq + 4 r =
// position 16 hq + r + 4 t (chunk256_bin).  The spectra wait in the lane's own slots of the wave tile during the
// component loop; Z, inverse pass 2, the exchange and inverse pass 1 run the same way back, stores from registers.
// HM (models with means, gmm_cplx_bussgang.py:96-100, :256-264, :288): lp k-step u adds 2 Re(Y_u^* u_k,u) as two more
// MFMAs on the lane's own spectra (Re Y, Im Y of position 16 hq + u; a second accumulator), the filter two more
// accumulator sets (Re b, Im b) at the filter positions, Z = Y f + b: 3x the MFMAs, one wave per SIMD (512
// registers) and a larger per-wave LDS slot for the tail's partial exchange.
template <int OUT, bool HM>
__global__ __launch_bounds__(256, HM ? 1 : 2) void k_fft_wreg(long long B, long long ntiles, int lg2, int Kp,
                                                              const double2* __restrict__ y,
                                                              const double* __restrict__ pr,
                                                              const double* __restrict__ pur,
                                                              const double* __restrict__ pui,
                                                              const double* __restrict__ pc,
                                                              const double* __restrict__ pw,
                                                              const double* __restrict__ pbr,
                                                              const double* __restrict__ pbi,
                                                              double2* __restrict__ h, double* __restrict__ om,
                                                              double* __restrict__ os, float* __restrict__ oa) {
  constexpr int N = 64, NT = 4, NL = 8, NW = 8, RS = N + 1;
  constexpr int WS = HM ? 1664 : 16 * RS;  // double2 per wave slot: the tile, or the tail's (F, Br, Bi, m, s) rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* tw = reinterpret_cast<double2*>(smem);
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  double* etab = reinterpret_cast<double*>(tw + 128);  // 2^(j/32), j < 32
  double2* tl = tw + 144;                               // pass-1 lane twiddles
  double2* T = tw + 208 + wid * WS;
  for (int t = tid; t < 128; t += 256) {
    double sn, cs;
    sincospi(-(double)t / 128.0, &sn, &cs);
    tw[t] = make_double2(cs, sn);
  }
  exp2_tab_init(etab, tid);
  pass1_lane_tw(tl, 6, lg2, tid);
  __syncthreads();
  const int col = lane & 15, hq = lane >> 4;
  const int g1 = lane & 15, s0 = lane >> 4;  // pass-1 lane: observations s0 + 4 q, positions g1 + 16 j
  double2* Town = T + col * RS + 16 * hq;    // the lane's pass-2 points
  const int ncb = Kp >> 4;
  // tables, y and h through buffer descriptors (scalar registers); per-lane 32-bit offsets
  const __amdgpu_buffer_rsrc_t rpr = buf_rsrc(pr, (unsigned)(Kp * N * 8)), rpw = buf_rsrc(pw, (unsigned)(Kp * N * 8));
  const __amdgpu_buffer_rsrc_t rpc = buf_rsrc(pc, (unsigned)(Kp * 8));
  const __amdgpu_buffer_rsrc_t rur = buf_rsrc(pur, HM ? (unsigned)(Kp * N * 8) : 0u);
  const __amdgpu_buffer_rsrc_t rui = buf_rsrc(pui, HM ? (unsigned)(Kp * N * 8) : 0u);
  const __amdgpu_buffer_rsrc_t rbr = buf_rsrc(pbr, HM ? (unsigned)(Kp * N * 8) : 0u);
  const __amdgpu_buffer_rsrc_t rbi = buf_rsrc(pbi, HM ? (unsigned)(Kp * N * 8) : 0u);
  const unsigned ul16 = (unsigned)lane * 16;
  const unsigned yo = (unsigned)(s0 * N + g1) * 16;  // pass-1 lane: byte offset of (s0, g1) in a tile
  FW_STAMP_DECL
  const long long W = (long long)gridDim.x * 4;
  const long long nmain = (ntiles / W) * W;
  double2 v[16];  // y of a tile in the pass-1 layout: v[4 q + j] = y[s0 + 4 q][g1 + 16 j]
  auto load_y = [&](long long t) __attribute__((always_inline)) {
    const long long bb = t * 16;
    const int rr = (int)((B - bb) < 16 ? (B - bb) : 16);
    const __amdgpu_buffer_rsrc_t ry = buf_rsrc(y + bb * N, (unsigned)(rr * N * 16));  // rows past B read 0
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = buf_ld2(ry, yo + 256 * j, 4096 * q);
  };
  auto run_tile = [&](long long tile, int s0b, int bs, long long next, bool coop) __attribute__((always_inline)) {
    const long long b0 = tile * 16;
    const int rows = (int)((B - b0) < 16 ? (B - b0) : 16);
    if (coop) load_y(tile);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      fft64_pass1<false>(v + 4 * q, lg2, g1, tl);
#pragma unroll
      for (int j = 0; j < 4; ++j) T[(s0 + 4 * q) * RS + g1 + 16 * j] = v[4 * q + j];
    }
    wave_lds_sync();
    FW_STAMP(0);
    {
      double2 yv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) yv[i] = Town[i];
      fft_pass_low4<false>(yv, lg2, tw);
#pragma unroll
      for (int i = 0; i < 16; ++i) Town[i] = yv[i];  // the lane's own slots: no other lane reads them
    }
    // |Y|^2 of lp k-step u is the lane's own point u, re-derived from the spectra per use (two VALU per k-step keep
    // 32 registers free for the next tile's y)
    auto y2 = [&](int u, unsigned o) {
      const double2 q = Town[u + o];
      return q.x * q.x + q.y * q.y;
    };
    FW_STAMP(1);
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
    // c'_comp is added after the MFMAs, so its loads have the whole product to land
    // HM: the mean tables of a block are loaded at its start and consumed after its |Y|^2 (lp) or w (filter) MFMAs,
    // which cover their latency; only the r / w tables are prefetched a block ahead (register budget)
    auto lp_block = [&](int cb, const double2* ta) {
      double pcv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) pcv[r] = buf_ld1(rpc, (unsigned)(hq + 4 * r) * 8, (unsigned)cb * 128);
      f64x4 C;
#pragma unroll
      for (int r = 0; r < 4; ++r) C[r] = 0.0;
      unsigned o = 0;  // opaque zero: the spectra reads stay in the loop instead of being hoisted into registers
      asm volatile("" : "+v"(o));
      double2 ua[HM ? NL : 1], qa[HM ? NL : 1];
      if constexpr (HM) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          ua[i] = buf_ld2(rur, ul16, (unsigned)cb * NL * 1024 + 1024 * i);
          qa[i] = buf_ld2(rui, ul16, (unsigned)cb * NL * 1024 + 1024 * i);
        }
      }
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        C = mfma16x16x4d(ta[i].x, y2(2 * i, o), C);
        C = mfma16x16x4d(ta[i].y, y2(2 * i + 1, o), C);
      }
      if constexpr (HM) {  // + 2 Re(Y^* u): (2 Re u) Re Y + (2 Im u) Im Y on the lane's own points
        f64x4 D;
#pragma unroll
        for (int r = 0; r < 4; ++r) D[r] = 0.0;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const double2 q0 = Town[2 * i + o], q1 = Town[2 * i + 1 + o];
          D = mfma16x16x4d(ua[i].x, q0.x, D);
          D = mfma16x16x4d(qa[i].x, q0.y, D);
          D = mfma16x16x4d(ua[i].y, q1.x, D);
          D = mfma16x16x4d(qa[i].y, q1.y, D);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) C[r] += D[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) C[r] += pcv[r];
      return C;
    };
    // Softmax with a lagging shift m: the weights are e^(lp - m) with m moved (and F, s rescaled) only when a lane's
    // block maximum exceeds it by more than 32 nats -- weights stay below e^32, and after the first blocks the
    // whole wave skips the rescale (column maximum, one exp, 16 multiplies).  ssum is the lane's own partial sum
    // (its 4 components of each block); the column sum is taken once per tile.
    auto softmax = [&](const f64x4& C, double* e) {
      const double lm = fmax(fmax(C[0], C[1]), fmax(C[2], C[3]));
      if (__builtin_amdgcn_ballot_w64(lm > m + 32.0)) {
        const double bm = col_max4(lm);
        const double mn = (bm > m + 32.0) ? bm : m;  // the column's four lanes agree (same bm, same m)
        const double alpha = exp_nonpos(m - mn, etab);  // 1 where the shift stays, ~0 from -inf
        ssum *= alpha;
#pragma unroll
        for (int t = 0; t < NT; ++t) F[t] *= alpha;
        if constexpr (HM) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            Br[t] *= alpha;
            Bi[t] *= alpha;
          }
        }
        m = mn;
      }
      const double sh = (m == -__builtin_inf()) ? 0.0 : m;
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = exp_nonpos(C[r] - sh, etab);
      ssum += (e[0] + e[1]) + (e[2] + e[3]);
    };
    auto filter_block = [&](const double2* tb, int cb, const double* e) {
      double2 tr[HM ? NW : 1], ti[HM ? NW : 1];
      if constexpr (HM) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          tr[i] = buf_ld2(rbr, ul16, (unsigned)cb * NW * 1024 + 1024 * i);
          ti[i] = buf_ld2(rbi, ul16, (unsigned)cb * NW * 1024 + 1024 * i);
        }
      }
#pragma unroll
      for (int j = 0; j < 4 * NT; ++j) {
        const int r = j / NT, t = j % NT;
        const double wv = (j & 1) ? tb[j >> 1].y : tb[j >> 1].x;
        F[t] = mfma16x16x4d(wv, e[r], F[t]);
      }
      if constexpr (HM) {
#pragma unroll
        for (int j = 0; j < 4 * NT; ++j) {
          const int r = j / NT, t = j % NT;
          Br[t] = mfma16x16x4d((j & 1) ? tr[j >> 1].y : tr[j >> 1].x, e[r], Br[t]);
        }
#pragma unroll
        for (int j = 0; j < 4 * NT; ++j) {
          const int r = j / NT, t = j % NT;
          Bi[t] = mfma16x16x4d((j & 1) ? ti[j >> 1].y : ti[j >> 1].x, e[r], Bi[t]);
        }
      }
    };
    const int nb = (ncb - s0b + bs - 1) / bs;  // this wave's component blocks s0b + j bs, j < nb
    auto blk = [&](int j) { return s0b + j * bs; };
    if (nb > 0) {
      const int last = nb - 1;
      double2 ta[NL], tb[NW];
      auto load_lp = [&](int cb) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NL; ++i) ta[i] = buf_ld2(rpr, ul16, (unsigned)cb * NL * 1024 + 1024 * i);
      };
      auto load_w = [&](int cb) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NW; ++i) tb[i] = buf_ld2(rpw, ul16, (unsigned)cb * NW * 1024 + 1024 * i);
      };
      load_lp(blk(0));
      f64x4 C = lp_block(blk(0), ta);
      load_lp(blk(last > 0 ? 1 : 0));
      load_w(blk(0));
      FW_STAMP(2);
      for (int j = 0; j < last; ++j) {
        const int b1 = blk(j + 1), b2 = blk(j + 2 < last ? j + 2 : last);
        const f64x4 Cn = lp_block(b1, ta);
        load_lp(b2);
        double e[4];
        softmax(C, e);
        filter_block(tb, blk(j), e);
        load_w(b1);
        C = Cn;
      }
      FW_STAMP(3);
      if (next >= 0) load_y(next);  // behind the last block, the merge, the inverse transform and the store
      {
        double e[4];
        softmax(C, e);
        filter_block(tb, blk(last), e);
      }
    }
    ssum = col_sum4(ssum);  // the lanes' partial sums -> the column's (bit-identical in its four lanes)
    if (coop) {  // waves 1-3 hand (F, m, s) to wave 0 through their own tiles (wave 0's holds its spectra)
      double* Td = reinterpret_cast<double*>(T);
      constexpr int NA = HM ? 3 : 1;  // accumulator sets: F (, Br, Bi)
      if (wid != 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            Td[(t * 4 + r) * 64 + lane] = F[t][r];
            if constexpr (HM) {
              Td[(4 * NT + t * 4 + r) * 64 + lane] = Br[t][r];
              Td[(8 * NT + t * 4 + r) * 64 + lane] = Bi[t][r];
            }
          }
        Td[NA * 4 * NT * 64 + lane] = m;
        Td[(NA * 4 * NT + 1) * 64 + lane] = ssum;
      }
      __syncthreads();
      if (wid == 0) {  // fixed order: wave 0's own partial, then waves 1, 2, 3
        double mm = m;
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const double* Tw = reinterpret_cast<const double*>(tw + 208 + w * WS);
          mm = fmax(mm, Tw[NA * 4 * NT * 64 + lane]);
        }
        const double f0 = exp_nonpos(m - mm, etab);
        ssum *= f0;
#pragma unroll
        for (int t = 0; t < NT; ++t) F[t] *= f0;
        if constexpr (HM) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            Br[t] *= f0;
            Bi[t] *= f0;
          }
        }
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const double* Tw = reinterpret_cast<const double*>(tw + 208 + w * WS);
          const double mw = Tw[NA * 4 * NT * 64 + lane];
          const double fw = exp_nonpos(mw - mm, etab);
          ssum = fma(Tw[(NA * 4 * NT + 1) * 64 + lane], fw, ssum);
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              F[t][r] = fma(Tw[(t * 4 + r) * 64 + lane], fw, F[t][r]);
              if constexpr (HM) {
                Br[t][r] = fma(Tw[(4 * NT + t * 4 + r) * 64 + lane], fw, Br[t][r]);
                Bi[t][r] = fma(Tw[(8 * NT + t * 4 + r) * 64 + lane], fw, Bi[t][r]);
              }
            }
        }
        m = mm;
      }
    }
    if (!coop || wid == 0) {
      const double sc = (OUT == 0) ? 1.0 / ssum : 1.0;
      if ((OUT == 3 || OUT == 4) && hq == 0 && col < rows) {
        om[b0 + col] = m;
        os[b0 + col] = ssum;
      }
      double2 z[16];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double2 q = Town[r + 4 * t];
          const double f = F[t][r] * sc;
          if constexpr (HM)
            z[r + 4 * t] = make_double2(fma(q.x, f, Br[t][r] * sc), fma(q.y, f, Bi[t][r] * sc));
          else
            z[r + 4 * t] = make_double2(q.x * f, q.y * f);
        }
      FW_STAMP(4);
      fft_pass_low4<true>(z, lg2, tw);
#pragma unroll
      for (int i = 0; i < 16; ++i) Town[i] = z[i];
      wave_lds_sync();
      const unsigned ob = (unsigned)rows * N * 16;  // rows past B: stores dropped by the descriptor extent
      const __amdgpu_buffer_rsrc_t ro = (OUT == 0) ? buf_rsrc(h + b0 * N, ob)
                                      : (OUT == 3) ? buf_rsrc(reinterpret_cast<float2*>(oa) + b0 * N, ob / 2)
                                                   : buf_rsrc(reinterpret_cast<double2*>(oa) + b0 * N, ob);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double2 x[4];
        const int sr = s0 + 4 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = T[sr * RS + g1 + 16 * j];
        fft64_pass1<true>(x, lg2, g1, tl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (OUT == 3)
            buf_st1f2(make_float2((float)x[j].x, (float)x[j].y), ro, yo / 2 + 128 * j, 2048 * q);
          else
            buf_st2(x[j], ro, yo + 256 * j, 4096 * q);
        }
      }
      FW_STAMP(5);
    }
    if (coop) __syncthreads();  // wave 0 has read the partials before the next tile overwrites them
    wave_lds_sync();
    FW_STAMP(6);
  };
  long long tile = (long long)blockIdx.x * 4 + wid;
  if (tile < nmain) load_y(tile);
  for (; tile < nmain; tile += W) run_tile(tile, 0, 1, tile + W < nmain ? tile + W : -1, false);
  for (long long tt = nmain + blockIdx.x; tt < ntiles; tt += gridDim.x) run_tile(tt, wid, 4, -1, true);
  FW_STAMP_FLUSH
}

template <int OUT, bool HM>
hipError_t launch_wreg(const QceFftEstArgs& a, hipStream_t st) {
  const size_t lds = 128 * 16 + 32 * 8 + 64 * 16 + (size_t)4 * (HM ? 1664 : 16 * 65) * 16;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fft_wreg<OUT, HM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const long long ntiles = (a.B + 15) / 16;
  // persistent: two workgroups (8 waves) per CU, one with means (a wave per SIMD)
  const long long slots = (HM ? 1LL : 2LL) * (a.cu > 0 ? a.cu : 256);
  const long long wgs = ntiles < slots ? ntiles : slots;
  hipLaunchKernelGGL((k_fft_wreg<OUT, HM>), dim3((unsigned)wgs), dim3(256), lds, st, a.B, ntiles, __builtin_ctz(a.n2),
                     a.Kp, a.y, a.pr, a.pur, a.pui, a.pc, a.pw, a.pbr, a.pbi, a.h, a.om, a.os, a.oa);
  return hipGetLastError();
}

}  // namespace
