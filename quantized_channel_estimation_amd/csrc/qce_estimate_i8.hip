// Int8-slice (Ozaki) 'all'-mode estimate for quantised observations, padded M, N <= 64.
//
// After one scale y_scale the quantiser outputs are small integers ti (1 bit: +-1, uniform b-bit: odd, |ti| <= 2^b - 1),
// so the two table products of a component, E(Linv_k) y and E(W_k) y, run on v_mfma_i32_16x16x64_i8:
//  * k_pack_i8: every row r of a real-embedded table gets the frexp exponent e_r of its largest magnitude and
//    q = rint(T[r, :] 2^(7S-1-e_r)) (half to even), written in balanced base 128, digits in [-64, 63], least
//    significant first, the final carry folded into the top digit (<= 64): S int8 planes and one exponent per row.
//  * k_est_all_i8: acc_s = D_s ti in int32 (|acc_s| <= 64 127 128 < 2^21, exact).  Neighbouring planes are combined
//    in int32 by Horner steps acc = 128 acc + D_s ti through the MFMA's C operand (two planes: < 2^28; three at 1 bit:
//    < 2^28), the groups in FP64: raw = sum_s 128^s acc_s.  u = raw_L 2^(e_r-7S+1) / y_scale - q0, z = raw_W 2^(e_r-7S+1)
//    / y_scale + b, lp = c - sum u^2, online softmax over k and h = sum p z / sum p, all in FP64.
//
// Fragment use (16x16x64 i8): A = digits (row = lane & 15, 16 consecutive k bytes of k group lane >> 4), B = ti
// (column = sample = lane & 15, the same (lane group, byte) -> k assignment), D: col = lane & 15, row = 4 (lane >> 4)
// + reg.  The planes are stored fragment-major: one 1 KB block per (row block, plane, k step), lane l's 16 bytes at
// 16 l, so a wave's load of a fragment is one coalesced global_load_dwordx4 per lane.
//
// Work split: a workgroup of 4 waves owns a tile of 128 samples (8 blocks of 16, their ti resident in 8 VGPRs per
// block at 2MP = 128; 64 samples where padded M < 64 = padded N); wave w owns the 16-row blocks w, w + 4, ... of both tables, so every digit byte is read once
// per workgroup and component and the FP64 output state of a wave is its own rows only.  The quadratic form is summed
// over the waves through LDS (one barrier per component, two buffers), then every wave runs the same softmax update
// (its running max and sum live in LDS, one private slot per lane).  All S x k-step fragments of a row block are
// loaded at once, and the next block's loads are issued as soon as the block's MFMAs are done, under its FP64 epilogue.
//
// A sample with an observation off the grid (|t - rint(t)| > 2^-20 or |rint(t)| > 127) gets NaN in its whole row.
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "qce_kernels.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int NBMAX = 8;          // 16-sample blocks per workgroup tile (the kernel's NB: 8, or 4 where 8 do not fit)
constexpr int TILE = 16 * NBMAX;  // samples per workgroup at NB = 8
constexpr int WAVES = 4;

__host__ __device__ inline int i8_ksteps(int MP) { return 2 * MP > 64 ? (2 * MP) / 64 : 1; }

// bytes of one component's planes: (2MP + 2NP) / 16 row blocks x S planes x k steps x 1 KB
__host__ __device__ inline long long i8_plane_bytes(int MP, int NP, int S) {
  return (long long)((2 * MP + 2 * NP) / 16) * S * i8_ksteps(MP) * 1024;
}

// one thread per table row: blockIdx.x = component, blockIdx.y = 0 (E(Linv_k)) / 1 (E(W_k))
__global__ __launch_bounds__(128) void k_pack_i8(int M, int N, int MP, int NP, int S, double y_scale,
                                                 const double2* __restrict__ Linv, const double2* __restrict__ W,
                                                 const double2* __restrict__ q0, const double2* __restrict__ bvec,
                                                 signed char* __restrict__ planes, long long pstride,
                                                 double* __restrict__ rowtab, int* __restrict__ exps) {
  const int k = blockIdx.x, isW = blockIdx.y, r = threadIdx.x;
  const int RL = 2 * MP, RW = 2 * NP, KS = i8_ksteps(MP), KD = 64 * KS;
  const int rows_pad = isW ? RW : RL, rows = isW ? N : M;
  if (r >= rows_pad) return;
  const double2* Mx = isW ? W + (long long)k * N * M : Linv + (long long)k * M * M;
  const int i = r >> 1, rr = r & 1;
  auto value = [&](int c) -> double {
    const int j = c >> 1, cc = c & 1;
    if (i >= rows || j >= M) return 0.0;
    const double2 v = Mx[(long long)i * M + j];
    return (rr == cc) ? v.x : (rr == 0 ? -v.y : v.y);
  };
  double mx = 0.0;
  for (int c = 0; c < 2 * M; ++c) mx = fmax(mx, fabs(value(c)));
  int e = 0;
  if (mx > 0.0) (void)frexp(mx, &e);
  const int rb = (isW ? RL / 16 : 0) + r / 16, lr = r & 15;
  signed char* dst = planes + (long long)k * pstride + (long long)rb * S * KS * 1024;
  for (int c = 0; c < KD; ++c) {
    long long q = (long long)rint(ldexp(value(c), 7 * S - 1 - e));
    const int ks = c >> 6, g = (c & 63) >> 4, byte = c & 15;
    signed char* p = dst + (long long)ks * 1024 + (g * 16 + lr) * 16 + byte;
    for (int s = 0; s < S; ++s) {
      long long d = ((q + 64) & 127) - 64;  // balanced digit in [-64, 63]
      q = (q - d) >> 7;                     // exact: q - d is a multiple of 128
      if (s == S - 1) d += 128 * q;         // the final carry (0 or 1) goes into the top digit
      p[(long long)s * KS * 1024] = (signed char)d;
    }
  }
  // row tables: [scale_L (2MP) | q0 (2MP) | scale_W (2NP) | b (2NP)], exponents [L (2MP) | W (2NP)]
  double* rt = rowtab + (long long)k * (2 * RL + 2 * RW) + (isW ? 2 * RL : 0);
  rt[r] = ldexp(1.0, e - 7 * S + 1) / y_scale;
  double mean = 0.0;
  if (i < rows) {
    const double2 v = isW ? bvec[(long long)k * N + i] : q0[(long long)k * M + i];
    mean = rr ? v.y : v.x;
  }
  rt[rows_pad + r] = mean;
  exps[(long long)k * (RL + RW) + (isW ? RL : 0) + r] = e;
}

constexpr int SMAX = 8;  // most digit planes per table

// The S x KS fragments of one 16-row block (1 KB each, plane-major), all loads in flight at once; plane S - 1 (most
// significant) lands in a[0].  valid: wave-uniform.
template <int KS>
__device__ inline void load_block(const signed char* __restrict__ blk, int S, int lane, bool valid,
                                  v4i (&a)[SMAX][KS]) {
  if (!valid) return;
#pragma unroll
  for (int t = 0; t < SMAX; ++t)
    if (t < S) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        a[t][ks] = *reinterpret_cast<const v4i*>(blk + ((long long)(S - 1 - t) * KS + ks) * 1024 + lane * 16);
    }
}


// raw[j][reg] = sum over the S planes of one 16-row block for the sample blocks HB H + j, HB = NB / 2 blocks per pass
// (two passes over a row block's fragments bound the live accumulators).  G consecutive planes share
// an int32 accumulator (Horner steps acc = 128 acc + D ti through the MFMA's C operand), the groups fold into FP64.
template <int KS, int G, int H, int NB>
__device__ inline void block_products(const v4i (&a)[SMAX][KS], int S, const v4i (&ti)[NB][KS],
                                      double (&raw)[NB / 2][4]) {
  constexpr int HB = NB / 2;
  constexpr double F = G == 2 ? 16384.0 : 2097152.0;  // 128^G
  v4i acc[HB];
#pragma unroll
  for (int t = 0; t < SMAX; ++t)
    if (t < S) {
#pragma unroll
      for (int nb = 0; nb < HB; ++nb) {
        acc[nb] = t % G == 0 ? v4i{0, 0, 0, 0} : acc[nb] * 128;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc[nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t][ks], ti[HB * H + nb][ks], acc[nb], 0, 0, 0);
      }
      if (t % G == G - 1 || t == S - 1) {  // the group is complete: 128^(planes in it) = F, 128 F / ... for a short tail
        const double f = t % G == G - 1 ? F : (t % G == 0 ? 128.0 : 16384.0);
#pragma unroll
        for (int nb = 0; nb < HB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            raw[nb][q] = t < G ? (double)acc[nb][q] : fma(raw[nb][q], f, (double)acc[nb][q]);
      }
    }
}

// 16-sample blocks per workgroup: 8 (128 samples), 4 where the register file does not hold the state of 8
__host__ __device__ constexpr int i8_nb(int MP, int NP) { return MP < 64 && NP == 64 ? 4 : 8; }

// MP, NP: padded shape; G: planes per int32 group; DBG: write the raw sums of component a.dbg_k instead of h
template <int MP, int NP, int G, bool DBG>
__global__ __launch_bounds__(64 * WAVES, i8_nb(MP, NP) == 4 ? 2 : 1) void k_est_all_i8(const QceI8Args a) {
  constexpr int RL = 2 * MP / 16, RW = 2 * NP / 16;  // 16-row blocks of the two tables
  constexpr int IL = (RL + WAVES - 1) / WAVES, IW = (RW + WAVES - 1) / WAVES;
  constexpr int KS = 2 * MP > 64 ? (2 * MP) / 64 : 1;
  constexpr int NB = i8_nb(MP, NP), HB = NB / 2;
  __shared__ double qs[2][WAVES][TILE];
  __shared__ double ms[2 * NB][64 * WAVES];  // the softmax state (running max, sum) of a lane's NB samples
  __shared__ unsigned bads[64 * WAVES];      // ... and its off-grid flags: both are idle during the component loop
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, grp = lane >> 4;
  const long long b0 = (long long)blockIdx.x * (16 * NB);
  const int S = a.S;
  const long long bstride = (long long)S * KS * 1024;  // bytes of one row block's planes

  const int k0 = DBG ? a.dbg_k : 0, k1 = DBG ? a.dbg_k + 1 : a.K;
  // the digit fragments of the block in work; the next block's loads are issued as soon as its MFMAs are done
  v4i frag[SMAX][KS];
  load_block<KS>(a.planes + (long long)k0 * a.pstride + wave * bstride, S, lane, wave < RL, frag);

  // observations: ti of the tile's 8 sample blocks, the off-grid flags (bit nb: sample 16 nb + col)
  v4i ti[NB][KS];
  unsigned bad = 0;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const long long b = b0 + 16 * nb + col;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      int w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // complex elements 32 ks + 8 grp + e: bytes 2e (re), 2e + 1 (im)
        const int ci = 32 * ks + 8 * grp + e;
        if (b < a.B && ci < a.M) {
          const double2 v = a.y[b * a.M + ci];
          const double tr = v.x * a.y_scale, tm = v.y * a.y_scale;
          const double ir = rint(tr), im = rint(tm);
          const bool ok = fabs(tr - ir) <= 0x1p-20 && fabs(tm - im) <= 0x1p-20 && fabs(ir) <= 127.0 && fabs(im) <= 127.0;
          if (!ok) bad |= 1u << nb;
          const int br = ok ? (int)ir : 0, bi = ok ? (int)im : 0;
          w[e >> 1] |= ((br & 255) << (16 * (e & 1))) | ((bi & 255) << (16 * (e & 1) + 8));
        }
      }
      ti[nb][ks] = v4i{w[0], w[1], w[2], w[3]};
      __builtin_amdgcn_sched_barrier(0);  // one sample block's loads at a time: all in flight would fill the registers
    }
  }
  bad |= __shfl_xor((int)bad, 16);
  bad |= __shfl_xor((int)bad, 32);
  bads[threadIdx.x] = bad;

  double out[NB][IW][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    ms[2 * nb][threadIdx.x] = -INFINITY;
    ms[2 * nb + 1][threadIdx.x] = 0.0;
#pragma unroll
    for (int i = 0; i < IW; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[nb][i][q] = 0.0;
  }

  for (int k = k0; k < k1; ++k) {
    const signed char* pl = a.planes + (long long)k * a.pstride;
    const double* rt = a.rowtab + (long long)k * (4 * MP + 4 * NP);
    // log-prob product: this wave's row blocks of E(Linv_k), each in two passes of HB sample blocks
    double quad[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) quad[nb] = 0.0;
    auto fold_l = [&](auto hc, int rb, const double (&raw)[HB][4]) {
      constexpr int H = decltype(hc)::value;
      const int r0 = 16 * rb + 4 * grp;
      if (DBG) {
#pragma unroll
        for (int j = 0; j < HB; ++j) {
          const long long b = b0 + 16 * (HB * H + j) + col;
          if (b < a.B)
#pragma unroll
            for (int q = 0; q < 4; ++q) a.dbgL[b * (2 * MP) + r0 + q] = raw[j][q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double sc = rt[r0 + q], q0 = rt[2 * MP + r0 + q];
#pragma unroll
          for (int j = 0; j < HB; ++j) {
            const double u = raw[j][q] * sc - q0;
            quad[HB * H + j] = fma(u, u, quad[HB * H + j]);
          }
        }
      }
    };
#pragma unroll
    for (int i = 0; i < IL; ++i) {
      const int rb = wave + WAVES * i;
      double raw[HB][4];
      if (rb < RL) {
        block_products<KS, G, 0, NB>(frag, S, ti, raw);
        fold_l(std::integral_constant<int, 0>(), rb, raw);
        block_products<KS, G, 1, NB>(frag, S, ti, raw);
      }
      if (i + 1 < IL)
        load_block<KS>(pl + (rb + WAVES) * bstride, S, lane, rb + WAVES < RL, frag);
      else
        load_block<KS>(pl + (RL + wave) * bstride, S, lane, wave < RW, frag);
      if (rb < RL) fold_l(std::integral_constant<int, 1>(), rb, raw);
    }
    double p[NB], alpha[NB];
    if (!DBG) {
      // sum over the lane groups, then over the waves (fixed order: every wave gets the same bits)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        quad[nb] += __shfl_xor(quad[nb], 16);
        quad[nb] += __shfl_xor(quad[nb], 32);
      }
      if (grp == 0) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) qs[k & 1][wave][16 * nb + col] = quad[nb];
      }
      __syncthreads();
      const double ck = a.cconst[k];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        double qq = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) qq += qs[k & 1][w][16 * nb + col];
        const double lp = ck - qq;
        const double mold = ms[2 * nb][threadIdx.x];
        const double mnew = fmax(mold, lp);
        alpha[nb] = mold == mnew ? 1.0 : exp(mold - mnew);
        p[nb] = lp == mnew ? 1.0 : exp(lp - mnew);
        if (!(mnew > -INFINITY)) p[nb] = 0.0;
        ms[2 * nb + 1][threadIdx.x] = ms[2 * nb + 1][threadIdx.x] * alpha[nb] + p[nb];
        ms[2 * nb][threadIdx.x] = mnew;
      }
    }
    // filter product: this wave's row blocks of E(W_k)
#pragma unroll
    for (int i = 0; i < IW; ++i) {
      const int rb = wave + WAVES * i;
      auto fold_w = [&](auto hc, const double (&raw)[HB][4]) {
        constexpr int H = decltype(hc)::value;
        const int r0 = 16 * rb + 4 * grp;
        if (DBG) {
#pragma unroll
          for (int j = 0; j < HB; ++j) {
            const long long b = b0 + 16 * (HB * H + j) + col;
            if (b < a.B)
#pragma unroll
              for (int q = 0; q < 4; ++q) a.dbgW[b * (2 * NP) + r0 + q] = raw[j][q];
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double sc = rt[4 * MP + r0 + q], bq = rt[4 * MP + 2 * NP + r0 + q];
#pragma unroll
            for (int j = 0; j < HB; ++j) {
              const double z = raw[j][q] * sc + bq;
              out[HB * H + j][i][q] = fma(out[HB * H + j][i][q], alpha[HB * H + j], p[HB * H + j] * z);
            }
          }
        }
      };
      double raw[HB][4];
      if (rb < RW) {
        block_products<KS, G, 0, NB>(frag, S, ti, raw);
        fold_w(std::integral_constant<int, 0>(), raw);
        block_products<KS, G, 1, NB>(frag, S, ti, raw);
      }
      if (i + 1 < IW)
        load_block<KS>(pl + (RL + rb + WAVES) * bstride, S, lane, rb + WAVES < RW, frag);
      else
        load_block<KS>(pl + a.pstride + wave * bstride, S, lane, wave < RL && k + 1 < k1, frag);
      if (rb < RW) fold_w(std::integral_constant<int, 1>(), raw);
    }
  }
  if (DBG) return;
  // h: rows r0 .. r0 + 3 of the real embedding = complex elements r0 / 2, r0 / 2 + 1.  The row indices are computed
  // afresh from an opaque copy of the lane's column: shared with the prologue's they would stay live (and spill)
  // across the whole component loop.
  int col_out = col, grp_out = grp, tid_out = threadIdx.x;
  asm volatile("" : "+v"(col_out), "+v"(grp_out), "+v"(tid_out));
  const unsigned bad_out = bads[tid_out];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const long long b = b0 + 16 * nb + col_out;
    if (b >= a.B) continue;
    const bool isbad = (bad_out >> nb) & 1u;
    const double inv = 1.0 / ms[2 * nb + 1][tid_out];
#pragma unroll
    for (int i = 0; i < IW; ++i) {
      const int rb = wave + WAVES * i;
      if (rb >= RW) continue;
      const int n0 = 8 * rb + 2 * grp_out;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (n0 + c < a.N) {
          double2 v;
          v.x = isbad ? (double)NAN : out[nb][i][2 * c] * inv;
          v.y = isbad ? (double)NAN : out[nb][i][2 * c + 1] * inv;
          a.h[b * a.N + n0 + c] = v;
        }
      }
    }
  }
}

template <bool DBG>
hipError_t launch(const QceI8Args& a, hipStream_t st) {
  const dim3 block(64 * WAVES);
#define QCE_I8_CASE(mp, np)                                                        \
  if (a.MP == mp && a.NP == np) {                                                  \
    const dim3 grid((unsigned)((a.B + 16 * i8_nb(mp, np) - 1) / (16 * i8_nb(mp, np))));   \
    if (a.group == 3)                                                              \
      hipLaunchKernelGGL((k_est_all_i8<mp, np, 3, DBG>), grid, block, 0, st, a);   \
    else                                                                           \
      hipLaunchKernelGGL((k_est_all_i8<mp, np, 2, DBG>), grid, block, 0, st, a);   \
    return hipGetLastError();                                                      \
  }
  QCE_I8_CASE(16, 16)
  QCE_I8_CASE(16, 32)
  QCE_I8_CASE(16, 64)
  QCE_I8_CASE(32, 16)
  QCE_I8_CASE(32, 32)
  QCE_I8_CASE(32, 64)
  QCE_I8_CASE(64, 16)
  QCE_I8_CASE(64, 32)
  QCE_I8_CASE(64, 64)
#undef QCE_I8_CASE
  return hipErrorInvalidValue;
}

}  // namespace

bool qce_i8_shape(int MP, int NP) {
  return (MP == 16 || MP == 32 || MP == 64) && (NP == 16 || NP == 32 || NP == 64);
}

int qce_i8_tile(int MP, int NP) { return 16 * i8_nb(MP, NP); }

long long qce_pack_i8_bytes(int MP, int NP, int S) { return i8_plane_bytes(MP, NP, S); }

hipError_t qce_launch_pack_i8(int K, int M, int N, int MP, int NP, int S, double y_scale, const double2* Linv,
                              const double2* W, const double2* q0, const double2* bvec, signed char* planes,
                              double* rowtab, int* exps, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_i8, dim3(K, 2), dim3(128), 0, st, M, N, MP, NP, S, y_scale, Linv, W, q0, bvec, planes,
                     i8_plane_bytes(MP, NP, S), rowtab, exps);
  return hipGetLastError();
}

hipError_t qce_launch_est_i8(const QceI8Args& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  return a.dbgL ? launch<true>(a, st) : launch<false>(a, st);
}
