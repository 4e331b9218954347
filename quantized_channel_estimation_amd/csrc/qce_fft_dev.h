// Device helpers shared by the MFMA Fourier kernels (qce_fft_mfma.hip and the k_fft_* units it dispatches to):
// the LDS and register transforms, cross-row reductions, buffer-resource access, the table exp, the segment
// stamps of the diagnostic build, and the per-kernel launchers.
//
// FFTs: radix-2 DIF in LDS grouped into radix-8/4/2 register passes (natural order in, per-axis
// bit-reversed order out), the inverse is the exact reverse (DIT, conjugate twiddles), so no
// bit-reversal pass exists: the per-bin tables are stored in that bit-reversed order (k_fft_pack).
#pragma once
#include "qce_common.h"
#include "qce_kernels.h"

// One launcher per kernel unit; out: 0 'all' h, 3 / 4 K-shard partial (f32 / f64 accumulator)
hipError_t qce_fft_launch_wave(const QceFftEstArgs& a, int out, hipStream_t st);      // N = 16, 32
hipError_t qce_fft_launch_wreg(const QceFftEstArgs& a, int out, hipStream_t st);      // N = 64
hipError_t qce_fft_launch_chunk(const QceFftEstArgs& a, int out, hipStream_t st);     // N = 128, 256, zero mean
hipError_t qce_fft_launch_chunk_hm(const QceFftEstArgs& a, int out, hipStream_t st);  // N = 128, 256, with means

namespace {

constexpr double SQH = 0.70710678118654752440;  // sqrt(1/2)

QCE_DEV int brev(int j, int lg) { return lg == 0 ? 0 : (int)(__brev((unsigned)j) >> (32 - lg)); }

// v * e^{-2 pi i mm / P} (INV: e^{+...}); P in {2, 4, 8}, mm < P / 2 (compile-time after unrolling)
template <bool INV>
QCE_DEV double2 rootmul(double2 v, int P, int mm) {
  if (mm == 0) return v;
  if (P == 4 || mm == 2) return INV ? make_double2(-v.y, v.x) : make_double2(v.y, -v.x);
  if (mm == 1)
    return INV ? make_double2((v.x - v.y) * SQH, (v.x + v.y) * SQH) : make_double2((v.x + v.y) * SQH, (v.y - v.x) * SQH);
  return INV ? make_double2((-v.x - v.y) * SQH, (v.x - v.y) * SQH) : make_double2((v.y - v.x) * SQH, (-v.x - v.y) * SQH);
}

// One register pass of RL radix-2 stages over every line of one axis of every observation row.
// Axis length L = 2^lgL, element stride st (1: the n2 axis, n2: the n1 axis), first half-distance
// D = 2^lgD (axis units).  A group holds R = 2^RL elements a_m = blk 2D + j + m E (E = 2D / R).
// Forward (DIF): stage s pairs (m, m + R/2^{s+1}) with twiddle W_{2D_s}^{j + (m mod half) E}.
// Inverse (DIT): the same stages in reverse order, conjugate twiddles.
template <int RL, bool INV>
QCE_DEV void fft_pass(double2* T, int lgTS, int RS, int lgN, int lgL, int st, int lgD, const double2* tw, int t0,
                      int nthr) {
  constexpr int R = 1 << RL;
  const int lgE = lgD + 1 - RL;
  const int lgnb = lgL - lgD - 1;  // blocks per line
  const int total = 1 << (lgTS + lgN - RL);
  const int TSm = (1 << lgTS) - 1;
  for (int it = t0; it < total; it += nthr) {
    const int s = it & TSm, q = it >> lgTS;
    const int j = q & ((1 << lgE) - 1), rest = q >> lgE;
    const int blk = rest & ((1 << lgnb) - 1), line = rest >> lgnb;
    double2* row = T + s * RS;
    int idx[R];
    double2 x[R];
#pragma unroll
    for (int m = 0; m < R; ++m) {
      const int a = (blk << (lgD + 1)) + j + (m << lgE);
      idx[m] = (st == 1) ? (line << lgL) + a : a * st + line;
      x[m] = row[idx[m]];
    }
    double2 w[RL];
#pragma unroll
    for (int sI = 0; sI < RL; ++sI) {  // W_{2 D_s}^j = tw[j * 128 / D_s]
      w[sI] = tw[j << (7 - (lgD - sI))];
      if (INV) w[sI].y = -w[sI].y;
    }
    if (!INV) {
#pragma unroll
      for (int sI = 0; sI < RL; ++sI) {
        const int half = R >> (sI + 1);
#pragma unroll
        for (int m = 0; m < R; ++m) {
          if (m & half) continue;
          const double2 a = x[m], b = x[m + half];
          x[m] = cadd(a, b);
          x[m + half] = rootmul<false>(cmul(csub(a, b), w[sI]), 2 * half, m & (half - 1));
        }
      }
    } else {
#pragma unroll
      for (int sI = RL - 1; sI >= 0; --sI) {
        const int half = R >> (sI + 1);
#pragma unroll
        for (int m = 0; m < R; ++m) {
          if (m & half) continue;
          const double2 a = x[m];
          const double2 b = rootmul<true>(cmul(x[m + half], w[sI]), 2 * half, m & (half - 1));
          x[m] = cadd(a, b);
          x[m + half] = csub(a, b);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) row[idx[m]] = x[m];
  }
}

// Orders one wave's LDS accesses without a workgroup barrier: a wave's LDS instructions complete in
// issue order, so a compiler fence around the wave barrier is all the wave-local FFT passes need.
QCE_DEV void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// WAVE: the passes run over one wave's own tile (64 lanes, wave-local ordering); otherwise over the
// workgroup's tile (256 threads, __syncthreads between passes)
template <bool INV, bool WAVE = false>
QCE_DEV void fft_axis_passes(double2* T, int lgTS, int RS, int lgN, int lgL, int st, const double2* tw) {
  const int t0 = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x, nthr = WAVE ? 64 : 256;
  // forward: half-distances L/2 .. 1 in groups of <= 3 stages; inverse: the same passes reversed
  int rl[3], dd[3], np = 0;
  for (int rem = lgL, lgD = lgL - 1; rem > 0;) {
    const int r = rem < 3 ? rem : 3;
    rl[np] = r;
    dd[np] = lgD;
    ++np;
    lgD -= r;
    rem -= r;
  }
  for (int i = 0; i < np; ++i) {
    const int p = INV ? np - 1 - i : i;
    if (rl[p] == 3) fft_pass<3, INV>(T, lgTS, RS, lgN, lgL, st, dd[p], tw, t0, nthr);
    else if (rl[p] == 2) fft_pass<2, INV>(T, lgTS, RS, lgN, lgL, st, dd[p], tw, t0, nthr);
    else fft_pass<1, INV>(T, lgTS, RS, lgN, lgL, st, dd[p], tw, t0, nthr);
    if (WAVE) wave_lds_sync();
    else __syncthreads();
  }
}

// Diagnostic build only (-DQCE_STAMPS): per-wave cycle sums of a kernel's segments (s_memtime) into g_fft_stamps
// (qce_debug_fft_stamps); the product kernel executes no stamp.  The build has no relocatable device code, so every
// stamped kernel unit holds its own g_fft_stamps: FW_STAMP_UNIT(setter), placed before the kernel, defines the
// unit's pointer and the host function that sets it (qce_fft_set_stamps calls each unit's).
#ifdef QCE_STAMPS
#define FW_STAMP_UNIT(setter)                                                         \
  namespace {                                                                         \
  __device__ unsigned long long* g_fft_stamps = nullptr;                              \
  }                                                                                   \
  hipError_t setter(unsigned long long* dev) {                                        \
    return hipMemcpyToSymbol(HIP_SYMBOL(g_fft_stamps), &dev, sizeof(dev));            \
  }
#define FW_STAMP_DECL unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = __builtin_amdgcn_s_memtime();
#define FW_STAMP(i)                                             \
  do {                                                          \
    __builtin_amdgcn_sched_barrier(0);                          \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          \
    st_acc[(i)] += t_ - st_prev;                                \
    st_prev = t_;                                               \
    __builtin_amdgcn_sched_barrier(0);                          \
  } while (0)
#define FW_STAMP_FLUSH                                                                                  \
  if (g_fft_stamps && lane == 0 && blockIdx.x < 4096)                                                  \
    for (int i_ = 0; i_ < 8; ++i_) g_fft_stamps[((long long)blockIdx.x * 4 + wid) * 8 + i_] = st_acc[i_];
#else
#define FW_STAMP_UNIT(setter)
#define FW_STAMP_DECL
#define FW_STAMP(i)
#define FW_STAMP_FLUSH
#endif

// Reductions over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48) on the gfx950 cross-row
// swaps (no LDS round trip): op(swap pair) = op(x[l], x[l^16]) in either operand order, so every row of a
// column gets bit-identical results.
QCE_DEV void row_pair(double v, bool r32, double& a, double& b) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  if (r32) {
    const auto pl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto ph = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    a = __hiloint2double(ph[0], pl[0]);
    b = __hiloint2double(ph[1], pl[1]);
  } else {
    const auto pl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto ph = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    a = __hiloint2double(ph[0], pl[0]);
    b = __hiloint2double(ph[1], pl[1]);
  }
}
QCE_DEV double col_max4(double v) {
  double a, b;
  row_pair(v, false, a, b);
  row_pair(fmax(a, b), true, a, b);
  return fmax(a, b);
}
QCE_DEV double col_sum4(double v) {
  double a, b;
  row_pair(v, false, a, b);
  row_pair(a + b, true, a, b);
  return a + b;
}

// Buffer-resource memory access: a wave-uniform descriptor (base, byte extent) in scalar registers plus a 32-bit
// per-lane offset, so no 64-bit per-lane addresses occupy vector registers; loads past the extent return 0 and
// stores past it are dropped (the ragged last tile needs no guards).
typedef unsigned int qce_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int qce_u32x2 __attribute__((ext_vector_type(2)));
QCE_DEV __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
QCE_DEV double2 buf_ld2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
QCE_DEV double buf_ld1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
QCE_DEV void buf_st2(double2 v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(qce_u32x4, v), r, voff, soff, 0);
}
QCE_DEV void buf_st1f2(float2 v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qce_u32x2, v), r, voff, soff, 0);
}

// e^x for x <= 700 (x = -inf and x < -708 give e^-708 = 3e-308, negligible beside the largest weight 1, which every
// use has): 2^(k/32) from a 32-entry LDS
// table (exp2_tab, 2^(j/32)) times the degree-6 Taylor polynomial of e^r, |r| <= ln2/64 (truncation 4e-18), 2^(k>>5)
// added to the exponent field: 18 VALU against ~32 for the libm exp, about 2 ulp.
QCE_DEV double exp_nonpos(double x, const double* __restrict__ tab) {
  constexpr double L32 = 46.166241308446828384;      // 32 / ln 2
  constexpr double LH = 2.1660849390173098072e-02;   // ln 2 / 32, leading bits
  constexpr double LL = 2.3251928468788740148e-12;   // ln 2 / 32 - LH
  x = fmax(x, -708.0);  // -inf and deep underflow -> e^-708 (3e-308, negligible beside the largest weight 1)
  const double kf = __builtin_rint(x * L32);
  double r = fma(kf, -LH, x);
  r = fma(kf, -LL, r);
  const int k = (int)kf;
  double p = fma(r, 1.0 / 720.0, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const double v = tab[k & 31] * p;
  return __hiloint2double(__double2hiint(v) + ((k >> 5) << 20), __double2loint(v));
}
QCE_DEV void exp2_tab_init(double* tab, int tid) {
  if (tid < 32) tab[tid] = exp2((double)tid / 32.0);
}

// ---- register-resident transform of 16 points per thread (N = 256 in two passes of four radix-2 stages) ----
// v * e^{-2 pi i mm / 16} (INV: e^{+...}), mm < 8 compile-time after unrolling
template <bool INV>
QCE_DEV double2 rootmul16(double2 v, int mm) {
  if (!(mm & 1)) return rootmul<INV>(v, 8, mm >> 1);
  constexpr double C1 = 0.92387953251128675613, S1 = 0.38268343236508977173;  // cos, sin (pi / 8)
  const double c = (mm == 1) ? C1 : (mm == 3) ? S1 : (mm == 5) ? -S1 : -C1;
  const double s = (mm == 1) ? S1 : (mm == 3) ? C1 : (mm == 5) ? C1 : S1;  // sin(2 pi mm / 16)
  return INV ? make_double2(v.x * c - v.y * s, v.x * s + v.y * c) : make_double2(v.x * c + v.y * s, v.y * c - v.x * s);
}
template <bool INV>
QCE_DEV double2 root_any(double2 v, int P, int mm) {
  return P == 16 ? rootmul16<INV>(v, mm) : rootmul<INV>(v, P, mm);
}

// Radix-2^RL group on the registers x[S m], m < 2^RL: the stages of one contiguous bit range of one axis, first
// half-distance 2^lgD (axis units), j = the axis position bits below the range (the group twiddle W_{2D_s}^j;
// JZ: j == 0 for every thread).  Forward: DIF stages, inverse: the same stages reversed (DIT), conjugate twiddles --
// the arithmetic of fft_pass with all R elements in one thread.
// LT: tw is a pass-1 lane table (pass1_lane_tw) and j the lane's g: stage sI's twiddle is tw[16 sI + g].
template <int RL, bool INV, int S, bool JZ, bool LT = false>
QCE_DEV void reg_group(double2* x, int lgD, int j, const double2* tw) {
  constexpr int R = 1 << RL;
  double2 w[RL];
  if constexpr (!JZ) {
#pragma unroll
    for (int sI = 0; sI < RL; ++sI) {
      w[sI] = LT ? tw[16 * sI + j] : tw[j << (7 - (lgD - sI))];
      if (INV) w[sI].y = -w[sI].y;
    }
  }
  if constexpr (!INV) {
#pragma unroll
    for (int sI = 0; sI < RL; ++sI) {
      const int half = R >> (sI + 1);
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (m & half) continue;
        const double2 a = x[S * m], b = x[S * (m + half)];
        x[S * m] = cadd(a, b);
        double2 d = csub(a, b);
        if constexpr (!JZ) d = cmul(d, w[sI]);
        x[S * (m + half)] = root_any<false>(d, 2 * half, m & (half - 1));
      }
    }
  } else {
#pragma unroll
    for (int sI = RL - 1; sI >= 0; --sI) {
      const int half = R >> (sI + 1);
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (m & half) continue;
        const double2 a = x[S * m];
        double2 b = x[S * (m + half)];
        if constexpr (!JZ) b = cmul(b, w[sI]);
        b = root_any<true>(b, 2 * half, m & (half - 1));
        x[S * m] = cadd(a, b);
        x[S * (m + half)] = csub(a, b);
      }
    }
  }
}

// One pass over a thread's 2^RT points (array index = RT bits of the storage position): array bits [0, RA) are
// axis n2 (segment A), [RA, RT) axis n1 (segment B).  The axes are independent, so the segments run in either order.
template <int RT, int RA, bool INV, bool JZA, bool JZB, bool LT = false>
QCE_DEV void reg_pass(double2* x, int lgDA, int jA, int lgDB, int jB, const double2* tw) {
  constexpr int RB = RT - RA;
  if constexpr (RB > 0) {
#pragma unroll
    for (int a = 0; a < (1 << RA); ++a) reg_group<RB, INV, (1 << RA), JZB, LT>(x + a, lgDB, jB, tw);
  }
  if constexpr (RA > 0) {
#pragma unroll
    for (int b = 0; b < (1 << RB); ++b) reg_group<RA, INV, 1, JZA, LT>(x + (b << RA), lgDA, jA, tw);
  }
}
template <int RA, bool INV, bool JZA, bool JZB, bool LT = false>
QCE_DEV void reg_pass16(double2 (&x)[16], int lgDA, int jA, int lgDB, int jB, const double2* tw) {
  reg_pass<4, RA, INV, JZA, JZB, LT>(x, lgDA, jA, lgDB, jB, tw);
}

// Pass-1 lane twiddle table (64 double2): entry 16 sI + g = the stage-sI group twiddle of the lanes whose pass-1
// points have low bits g.  Read from the 128-entry table, pass 1 takes tw[j << (7 - (lgD - sI))] with j = g (or
// g >> lg2): the 16 lanes of a ds_read_b128 group (distinct g) land on only 2-8 of that table's bank quads (4- to
// 8-way conflicts, a quarter of the Fourier kernels' LDS cycles); the lane table puts them on 16 consecutive 16-byte
// slots.  The entries are computed like tw (same sincospi of the same index), so the values are the same.  The non-JZ
// segment of pass 1 is n2 bits [4, lg2) (j = g, lgD = lg2 - 1) for lg2 > 4, else n1 bits [4, lgN) (j = g >> lg2,
// lgD = lgN - 1 - lg2); threads 0-63 fill it.
QCE_DEV void pass1_lane_tw(double2* tl, int lgN, int lg2, int tid) {
  if (tid >= 64) return;
  const int sI = tid >> 4, g = tid & 15;
  const int RL = lg2 > 4 ? lg2 - 4 : (lg2 == 4 ? 0 : lgN - 4);
  const int lgD = lg2 > 4 ? lg2 - 1 : lgN - 1 - lg2;
  const int j = lg2 > 4 ? g : (g >> lg2);
  double sn = 0.0, cs = 1.0;
  if (sI < RL) sincospi(-(double)(j << (7 - (lgD - sI))) / 128.0, &sn, &cs);
  tl[tid] = make_double2(cs, sn);
}

// N = 64 = n1 n2: pass 1 = storage bits 5, 4 on a group of 4 points sharing the bits 0-3 (g); segment A = n2 bits
// [4, min(lg2, 6)), B = n1 bits [max(lg2, 4), 6), j = the axis bits below the segment
// tl: the pass-1 lane table (pass1_lane_tw with lgN = 6), indexed by g
template <bool INV>
QCE_DEV void fft64_pass1(double2* x, int lg2, int g, const double2* tl) {
  switch (lg2) {
    case 6: reg_pass<2, 2, INV, false, true, true>(x, 5, g, 0, 0, tl); break;
    case 5: reg_pass<2, 1, INV, false, true, true>(x, 4, g, 0, 0, tl); break;
    case 4: reg_pass<2, 0, INV, true, true, true>(x, 0, 0, 1, 0, tl); break;
    default: reg_pass<2, 0, INV, true, false, true>(x, 0, 0, 5 - lg2, g, tl); break;
  }
}

// N = 256 = n1 n2 (lg2 = log2 n2): the forward transform's stages in descending storage bit order are bits 7..4
// (pass 1) and 3..0 (pass 2) -- per axis high bits before low bits, as DIF requires.  Pass 1: the thread's points
// share the storage bits 0-3 (g), pass 2 the bits 4-7.
template <bool INV>  // tl: the pass-1 lane table (pass1_lane_tw with lgN = 8), indexed by g
QCE_DEV void fft256_pass1(double2 (&x)[16], int lg2, int g, const double2* tl) {
  switch (lg2) {  // segment A = n2 bits [4, lg2), B = n1 bits [max(lg2, 4), 8)
    case 8: reg_pass16<4, INV, false, true, true>(x, 7, g, 0, 0, tl); break;
    case 7: reg_pass16<3, INV, false, true, true>(x, 6, g, 0, 0, tl); break;
    case 6: reg_pass16<2, INV, false, true, true>(x, 5, g, 1, 0, tl); break;
    case 5: reg_pass16<1, INV, false, true, true>(x, 4, g, 2, 0, tl); break;
    case 4: reg_pass16<0, INV, true, true, true>(x, 0, 0, 3, 0, tl); break;
    default:  // n1 bits 4-7: the lane table holds the twiddles of j = the n1 bits < 4 at index g
      reg_pass16<0, INV, true, false, true>(x, 0, 0, 7 - lg2, g, tl);
      break;
  }
}
// pass 2 of every N >= 16 split: storage bits 3..0 of a lane's 16 points (bits >= 4 fixed)
template <bool INV>
QCE_DEV void fft_pass_low4(double2 (&x)[16], int lg2, const double2* tw) {
  switch (lg2 >= 4 ? 4 : lg2) {  // segment A = n2 bits [0, min(lg2, 4)), B = n1 bits [lg2, 4)
    case 4: reg_pass16<4, INV, true, true>(x, 3, 0, 0, 0, tw); break;
    case 3: reg_pass16<3, INV, true, true>(x, 2, 0, 0, 0, tw); break;
    case 2: reg_pass16<2, INV, true, true>(x, 1, 0, 1, 0, tw); break;
    case 1: reg_pass16<1, INV, true, true>(x, 0, 0, 2, 0, tw); break;
    default: reg_pass16<0, INV, true, true>(x, 0, 0, 3, 0, tw); break;
  }
}

// Filter-phase bin of k_fft_chunk<256>: wave w = t / 4 owns the storage positions with bits 4-7 = hq + 4 w, its tile
// t % 4 and accumulator register r (row hq + 4 r) give bits 0-3 = r + 4 (t % 4) -- exactly the 16 points a lane
// holds after pass 2, so the spectra and Z never pass through LDS between the transforms and the filter.
QCE_DEV int chunk256_bin(int t, int row) { return (((row & 3) + 4 * (t >> 2)) << 4) | ((row >> 2) + 4 * (t & 3)); }

}  // namespace
